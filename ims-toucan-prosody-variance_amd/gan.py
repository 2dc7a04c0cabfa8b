"""The speaker-embedding GAN's generator on the HIP kernels: ResNet_G of the reference's
InferenceInterfaces/Controllability/wgan/resnet_1.py (:8-80, ResNetBlock :133-181), in eval mode, fp32.

``pack_generator`` turns the checkpoint's ``generator_state_dict`` (``module.``-prefixed, as ``nn.DataParallel`` saves it, or not)
and ``model_parameters`` into a plan of ``tts_gan_conv2d`` launches (include/toucan_gan.h), one per layer:

* ``fc`` -> BatchNorm1d -> LeakyReLU(0.2): a 1x1 convolution of a 1x1 image, BatchNorm folded into scale and shift, rows permuted
  from the reference's (c, h, w) order to NHWC so that the result is the [N, 4, 4, nf0] image;
* every ResNetBlock: the learned shortcut (conv1x1 + BN, only when fin != fout) as its own launch, conv_0 + BN + LeakyReLU, and
  conv_1 + BN with the residual ``LeakyReLU(x_s + 0.1 dx)`` fused into its epilogue.  The ``Upsample(x2)`` after a block is never
  materialised: the next block reads its input (and an identity shortcut) through the kernel's upsampled load;
* ``conv_img`` (bias) -> LeakyReLU, then ``fc_out`` as a 1x1 convolution of a 1x1 image whose input columns are permuted from the
  reference's NCHW flattening to the NHWC one.

``GeneratorEngine.forward(z)`` runs the plan in chunks; ``intermediate(z)`` runs ``fc`` alone with the reference's row order and
returns ``l_1`` (the post-LeakyReLU output), which is all that ``GanWrapper.compute_controllability`` uses.
"""
import ctypes as C

import numpy as np
import torch

from . import capi

SLOPE = 0.2  # nn.LeakyReLU(0.2) of ResNet_G and ResNetBlock
RES_RATIO = 0.1  # ResNet_G(res_ratio=0.1): init_resnet passes none
BN_EPS = 1e-5
S0 = 4  # ResNet_G.s0
ACT_BUDGET_FLOATS = 1 << 26  # a chunk's largest activation stays within 256 MB


def _strip_prefix(sd):
    keys = list(sd)
    if keys and all(k.startswith("module.") for k in keys):
        return {k[len("module."):]: v for k, v in sd.items()}
    return dict(sd)


def _np(v):
    return (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float64)


def architecture(params):
    """(z_dim, data_dim, size, nf0, blocks) of ResNet_G(data_dim[-1], z_dim, size, nfilter, nfilter_max) (resnet_1.py:10-50):
    blocks = [(state-dict index, fin, fout, upsampled input)] in order.  Raises ValueError for what the engine cannot run."""
    if params.get("model") != "resnet":
        raise ValueError(f"model_parameters['model'] = {params.get('model')!r}: only 'resnet' exists (init_wgan.py:8-11)")
    for k in ("data_dim", "z_dim", "size", "nfilter", "nfilter_max"):
        if k not in params:
            raise ValueError(f"model_parameters has no {k!r}")
    size, nf, nf_max = int(params["size"]), int(params["nfilter"]), int(params["nfilter_max"])
    if size < 4 or size & (size - 1):
        raise ValueError(f"size = {size}: the generator needs a power of two >= 4")
    if nf < 1 or nf_max < 1:
        raise ValueError(f"nfilter = {nf}, nfilter_max = {nf_max}: both must be positive")
    if nf > nf_max:  # conv_img takes nfilter channels, the last block gives min(nfilter, nfilter_max): ResNet_G cannot run
        raise ValueError(f"nfilter = {nf} > nfilter_max = {nf_max}: conv_img would not match the last block's width")
    nlayers = int(np.log2(size / S0))
    nf0 = min(nf_max, nf * 2 ** (nlayers + 1))
    blocks, idx = [], 0
    for i in range(nlayers, 0, -1):
        blocks.append((idx, min(nf * 2 ** (i + 1), nf_max), min(nf * 2 ** i, nf_max), idx > 0))
        idx += 2  # ResNetBlock, Upsample
    blocks.append((idx, min(nf * 2, nf_max), min(nf, nf_max), idx > 0))
    blocks.append((idx + 1, min(nf, nf_max), min(nf, nf_max), False))
    return int(params["z_dim"]), int(params["data_dim"][-1]), size, nf0, blocks


def expected_shapes(params):
    """Every key of ResNet_G's state dict (unprefixed) -> its shape."""
    z_dim, data_dim, size, nf0, blocks = architecture(params)
    nf = int(params["nfilter"])

    def bn(p, c):
        return {p + ".weight": (c,), p + ".bias": (c,), p + ".running_mean": (c,), p + ".running_var": (c,), p + ".num_batches_tracked": ()}

    shapes = {"fc.weight": (nf0 * S0 * S0, z_dim), "fc.bias": (nf0 * S0 * S0,)}
    shapes.update(bn("bn1d", nf0 * S0 * S0))
    for idx, fin, fout, _ in blocks:
        p, fh = f"resnet.{idx}.", min(fin, fout)
        shapes[p + "conv_0.weight"] = (fh, fin, 3, 3)
        shapes.update(bn(p + "bn2d_0", fh))
        shapes[p + "conv_1.weight"] = (fout, fh, 3, 3)
        shapes.update(bn(p + "bn2d_1", fout))
        if fin != fout:
            shapes[p + "conv_s.weight"] = (fout, fin, 1, 1)
            shapes.update(bn(p + "bn2d_s", fout))
    shapes.update({"conv_img.weight": (3, nf, 3, 3), "conv_img.bias": (3,),
                   "fc_out.weight": (data_dim, 3 * size * size), "fc_out.bias": (data_dim,)})
    return shapes


def fold_bn(sd, p, bias=None):
    """Eval BatchNorm (eps 1e-5) after an optional bias as y = scale * acc + shift, folded in float64."""
    s = _np(sd[p + ".weight"]) / np.sqrt(_np(sd[p + ".running_var"]) + BN_EPS)
    b = 0.0 if bias is None else bias
    return s, s * (b - _np(sd[p + ".running_mean"])) + _np(sd[p + ".bias"])


def pack_weight(w):
    """torch conv weight [cout, cin, k, k] (or Linear [out, in]) -> [taps][cin_pad][cout_pad] fp32, zero padded (toucan_gan.h)."""
    w = np.asarray(w, dtype=np.float64)
    if w.ndim == 2:
        w = w[:, :, None, None]
    cout, cin, k, _ = w.shape
    cin_pad = -(-cin // capi.GAN_KC) * capi.GAN_KC
    cout_pad = -(-cout // capi.GAN_NC) * capi.GAN_NC
    out = np.zeros((k * k, cin_pad, cout_pad), np.float32)
    out[:, :cin, :cout] = w.transpose(2, 3, 1, 0).reshape(k * k, cin, cout)
    return out


def nchw_to_nhwc_perm(c, h):
    """perm[j] = the (c, h, w)-flattened index of NHWC position j = (y * h + x) * c + ch."""
    return np.arange(c * h * h).reshape(c, h * h).T.reshape(-1)


def _layer(name, w, scale, shift, h, src, flags=0, res=None):
    w = np.asarray(w, dtype=np.float64)
    cout, cin = w.shape[0], w.shape[1]
    return dict(name=name, w=pack_weight(w), scale=None if scale is None else np.asarray(scale, np.float32),
                shift=None if shift is None else np.asarray(shift, np.float32), cin=cin, cout=cout,
                taps=1 if w.ndim == 2 else w.shape[2] * w.shape[3], h=h, src=src, res=res, flags=flags)


def pack_generator(state_dict, params):
    """The launch plan of ResNet_G for ``tts_gan_conv2d``.  Layer ``src`` / ``res``: the index of the layer whose output is read
    (-1: the latent).  Raises ValueError for parameters it cannot run and for missing, unexpected or misshapen keys."""
    z_dim, data_dim, size, nf0, blocks = architecture(params)
    sd = _strip_prefix(state_dict)
    shapes = expected_shapes(params)
    missing = sorted(set(shapes) - set(sd))
    if missing:
        raise ValueError(f"generator_state_dict lacks {len(missing)} keys: {missing[:6]}")
    unexpected = sorted(set(sd) - set(shapes))
    if unexpected:
        raise ValueError(f"generator_state_dict has unexpected keys: {unexpected[:6]}")
    for k, shp in shapes.items():
        if tuple(np.shape(_np(sd[k]))) != shp:
            raise ValueError(f"{k}: shape {tuple(np.shape(_np(sd[k])))}, expected {shp}")

    lrelu = capi.GAN_LRELU
    fc_w, fc_b = _np(sd["fc.weight"]), _np(sd["fc.bias"])
    scale, shift = fold_bn(sd, "bn1d", fc_b)
    perm = nchw_to_nhwc_perm(nf0, S0)
    fc_nhwc = _layer("fc", fc_w[perm], scale[perm], shift[perm], 1, -1, lrelu)
    layers, h, x = [fc_nhwc], S0, 0
    for idx, fin, fout, upsampled in blocks:
        p = f"resnet.{idx}."
        if upsampled:
            h *= 2
        up = capi.GAN_UPSAMPLE if upsampled else 0
        if fin != fout:
            sc, sh = fold_bn(sd, p + "bn2d_s")
            layers.append(_layer(p + "conv_s", _np(sd[p + "conv_s.weight"]), sc, sh, h, x, up))
            res, res_flags = len(layers) - 1, 0
        else:
            res, res_flags = x, capi.GAN_RES_UPSAMPLE if upsampled else 0
        sc, sh = fold_bn(sd, p + "bn2d_0")
        layers.append(_layer(p + "conv_0", _np(sd[p + "conv_0.weight"]), sc, sh, h, x, up | lrelu))
        sc, sh = fold_bn(sd, p + "bn2d_1")
        layers.append(_layer(p + "conv_1", _np(sd[p + "conv_1.weight"]), sc, sh, h, len(layers) - 1,
                             capi.GAN_RESIDUAL | res_flags | lrelu, res=res))
        x = len(layers) - 1
    layers.append(_layer("conv_img", _np(sd["conv_img.weight"]), None, _np(sd["conv_img.bias"]), h, x, lrelu))
    fo_w = _np(sd["fc_out.weight"])[:, nchw_to_nhwc_perm(3, size)]
    layers.append(_layer("fc_out", fo_w, None, _np(sd["fc_out.bias"]), 1, len(layers) - 1))
    # the intermediate: fc in the reference's row order, so that l_1 comes out as ResNet_G returns it
    fc_ref = _layer("fc_ref", fc_w, scale, shift, 1, -1, lrelu)
    return dict(z_dim=z_dim, data_dim=data_dim, size=size, nf0=nf0, layers=layers, fc_ref=fc_ref)


def layer_out_floats(layer):
    """Floats one sample's output of a layer takes (the 1x1-image layers hold their whole vector in the channels)."""
    return layer["h"] * layer["h"] * layer["cout"]


class GeneratorEngine:
    """ResNet_G.forward (eval) on the GPU.  ``forward(z) -> [N, data_dim]``; ``intermediate(z) -> [N, nf0 * 16]``.  Every sample is
    computed in an order of its own: the results do not depend on N, the chunk size or the sample's place in the batch."""

    def __init__(self, state_dict, params, device, chunk=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise capi.ToucanHipError(f"GeneratorEngine needs a GPU device, got {device!r} (the generator has no CPU path)")
        self.lib = capi.lib()
        self.plan = pack_generator(state_dict, params)
        self.z_dim, self.data_dim, self.nf0 = self.plan["z_dim"], self.plan["data_dim"], self.plan["nf0"]
        self.layers = [self._upload(l) for l in self.plan["layers"]]
        self.fc_ref = self._upload(self.plan["fc_ref"])
        per_sample = max(layer_out_floats(l) for l in self.layers)
        self.chunk = int(chunk) if chunk else max(1, ACT_BUDGET_FLOATS // per_sample)

    def _upload(self, layer):
        d = dict(layer)
        for k in ("w", "scale", "shift"):
            d[k] = None if layer[k] is None else torch.from_numpy(layer[k]).to(self.device)
        return d

    def _launch(self, layer, x, n, res=None):
        y = torch.empty((n * layer["h"] * layer["h"], layer["cout"]), dtype=torch.float32, device=self.device)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        desc = capi.TtsGanConvDesc(x=ptr(x), w=ptr(layer["w"]), scale=ptr(layer["scale"]), shift=ptr(layer["shift"]), res=ptr(res),
                                   y=ptr(y), n=n, h=layer["h"], cin=layer["cin"], cout=layer["cout"], taps=layer["taps"],
                                   flags=layer["flags"], pre_slope=SLOPE, res_ratio=RES_RATIO, slope=SLOPE)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.check(self.lib.tts_gan_conv2d(C.byref(desc), C.c_void_p(stream)), layer["name"])
        return y

    def _latents(self, z):
        z = torch.as_tensor(z)
        if z.dim() != 2 or z.shape[1] != self.z_dim:
            raise ValueError(f"latents of shape {tuple(z.shape)}, expected [N, {self.z_dim}]")
        return z.to(device=self.device, dtype=torch.float32).contiguous()

    def forward_chunk(self, z):
        """One pass of the plan over z [n, z_dim] (on the device)."""
        n, outs = z.shape[0], []
        for layer in self.layers:
            x = z if layer["src"] < 0 else outs[layer["src"]]
            outs.append(self._launch(layer, x, n, None if layer["res"] is None else outs[layer["res"]]))
        return outs[-1]

    def forward(self, z):
        z = self._latents(z)
        if z.shape[0] <= self.chunk:
            return self.forward_chunk(z)
        out = torch.empty((z.shape[0], self.data_dim), dtype=torch.float32, device=self.device)
        for b in range(0, z.shape[0], self.chunk):
            out[b:b + self.chunk] = self.forward_chunk(z[b:b + self.chunk])
        return out

    __call__ = forward

    def intermediate(self, z):
        """l_1 of ResNet_G.forward(z, return_intermediate=True): fc -> BatchNorm1d -> LeakyReLU, in the reference's (c, h, w) order."""
        z = self._latents(z)
        return self._launch(self.fc_ref, z, z.shape[0])
