"""CPU tests of the speaker-embedding GAN's host side (gan.py, controllable.py, the fixture checkpoint): the packed launch plan,
restated in numpy (tests/gan_ref.py), against the reference's ResNet_G (tests/golden/gan/gan.npz); the checkpoint layout; BatchNorm
folding; the fc_out permutation; the checks; the seeded GanWrapper arithmetic; the C ABI of include/toucan_gan.h."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ims_toucan_prosody_variance_amd  # noqa: F401
from ims_toucan_prosody_variance_amd import capi, controllable, fixture_weights as fw, gan, interface
from tests import gan_ref as gr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, "tests", "golden", "gan", "gan.npz"))
VARIANTS = json.loads(str(G["variants"]))


def _checkpoint(name, tmp):
    params = json.loads(str(G[f"{name}/params"]))
    path = interface.write_fixture_gan_checkpoint(str(tmp), params=params, seed=int(G[f"{name}/ckpt_seed"]))
    return path, torch.load(path, weights_only=True)


@pytest.mark.parametrize("name", VARIANTS)
def test_plan_restatement_matches_reference(name, tmp_path):
    _, ck = _checkpoint(name, tmp_path)
    plan = gan.pack_generator(ck["generator_state_dict"], ck["model_parameters"])
    y64 = G[f"{name}/y64"]
    y = gr.run_plan(plan, G[f"{name}/z"])
    assert np.abs(y - y64).max() <= 1e-6 * np.abs(y64).max()
    l1 = gr.intermediate(plan, G[f"{name}/z"][:G[f"{name}/l1_64"].shape[0]])
    assert np.abs(l1 - G[f"{name}/l1_64"]).max() <= 1e-6 * np.abs(G[f"{name}/l1_64"]).max()


def test_checkpoint_layout(tmp_path):
    path, ck = _checkpoint("s16cap", tmp_path)
    assert path.endswith(os.path.join("Embedding", "embedding_gan.pt"))
    assert set(ck) == {"model_parameters", "generator_state_dict", "critic_state_dict", "dataset_mean", "dataset_std"}
    p = ck["model_parameters"]
    assert p["model"] == "resnet" and p["z_dim"] == 32 and isinstance(p["data_dim"], tuple) and len(p["data_dim"]) == 3
    for sd in (ck["generator_state_dict"], ck["critic_state_dict"]):
        assert all(k.startswith("module.") for k in sd)
    g = ck["generator_state_dict"]
    assert "module.resnet.4.conv_s.weight" in g and "module.resnet.0.conv_s.weight" not in g  # 32 -> 32: identity shortcut
    assert "module.fc_input.weight" in ck["critic_state_dict"]
    # non-trivial BatchNorm statistics and affine terms, so that folding them is tested
    for bn in ("bn1d", "resnet.0.bn2d_0", "resnet.4.bn2d_s"):
        assert g[f"module.{bn}.running_var"].std() > 0.1 and g[f"module.{bn}.running_mean"].abs().mean() > 0.05
        assert g[f"module.{bn}.weight"].std() > 0.05 and g[f"module.{bn}.bias"].abs().mean() > 0.02
    assert ck["dataset_mean"].shape == (64,) and ck["dataset_std"].shape == (64,)


def test_prefixed_and_unprefixed_keys_pack_alike(tmp_path):
    _, ck = _checkpoint("s8", tmp_path)
    a = gan.pack_generator(ck["generator_state_dict"], ck["model_parameters"])
    b = gan.pack_generator({k[len("module."):]: v for k, v in ck["generator_state_dict"].items()}, ck["model_parameters"])
    for la, lb in zip(a["layers"] + [a["fc_ref"]], b["layers"] + [b["fc_ref"]]):
        assert np.array_equal(la["w"], lb["w"]) and la["name"] == lb["name"]


def test_bn_folding_matches_eval_batchnorm():
    rng = np.random.default_rng(3)
    c = 40
    sd = {"bn.weight": rng.uniform(0.5, 1.5, c), "bn.bias": rng.normal(0, 0.3, c), "bn.running_mean": rng.normal(0, 0.5, c),
          "bn.running_var": rng.uniform(0.2, 2.0, c)}
    acc, bias = rng.normal(0, 2, (7, c)), rng.normal(0, 0.4, c)
    scale, shift = gan.fold_bn(sd, "bn", bias)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ref = torch.nn.functional.batch_norm(t(acc + bias), t(sd["bn.running_mean"]), t(sd["bn.running_var"]), t(sd["bn.weight"]),
                                         t(sd["bn.bias"]), False, 0.0, 1e-5).numpy()
    np.testing.assert_allclose(acc * scale + shift, ref, rtol=1e-12, atol=1e-12)


def test_fc_out_and_fc_permutations():
    rng = np.random.default_rng(4)
    for c, h in ((3, 8), (7, 4)):
        img = rng.normal(size=(2, c, h, h))  # NCHW, as the reference flattens it
        perm = gan.nchw_to_nhwc_perm(c, h)
        nhwc = img.transpose(0, 2, 3, 1).reshape(2, -1)
        assert np.array_equal(img.reshape(2, -1)[:, perm], nhwc)
    # fc_out with permuted columns on the NHWC image == the reference's fc_out on the NCHW flattening
    w = rng.normal(size=(5, 3 * 16))
    img = rng.normal(size=(1, 3, 4, 4))
    np.testing.assert_allclose(w[:, gan.nchw_to_nhwc_perm(3, 4)] @ img.transpose(0, 2, 3, 1).reshape(-1), w @ img.reshape(-1))


def test_pack_weight_layout():
    w = np.arange(5 * 3 * 3 * 3, dtype=np.float64).reshape(5, 3, 3, 3)  # [cout][cin][ky][kx], asymmetric
    p = gan.pack_weight(w)
    assert p.shape == (9, 16, 64) and not p[:, 3:].any() and not p[:, :, 5:].any()
    for ky in range(3):
        for kx in range(3):
            assert np.array_equal(p[3 * ky + kx, :3, :5], w[:, :, ky, kx].T)


@pytest.mark.parametrize("change, match", [
    (dict(size=12), "power of two"), (dict(size=2), "power of two"), (dict(model="dcgan"), "resnet"),
    (dict(nfilter=64, nfilter_max=32), "nfilter"), (dict(z_dim=None), "z_dim"),
])
def test_unsupported_parameters_raise(change, match):
    params = dict(fw.GAN_PARAMS, **change)
    params = {k: v for k, v in params.items() if v is not None}
    with pytest.raises(ValueError, match=match):
        gan.pack_generator({}, params)


def test_missing_unexpected_and_misshapen_keys_raise():
    params = dict(fw.GAN_PARAMS, size=8, nfilter=8, nfilter_max=32)
    g, _ = fw.gan_state_dicts(params, 1)
    gan.pack_generator(g, params)
    with pytest.raises(ValueError, match="lacks"):
        gan.pack_generator({k: v for k, v in g.items() if "bn2d_1.running_var" not in k}, params)
    with pytest.raises(ValueError, match="unexpected"):
        gan.pack_generator(dict(g, **{"module.extra.weight": np.zeros(3)}), params)
    with pytest.raises(ValueError, match="shape"):
        gan.pack_generator(dict(g, **{"module.fc_out.bias": np.zeros(65)}), params)


class _PlanGenerator:
    """gan.GeneratorEngine's interface on the float64 restatement (no GPU): lets GanWrapper's own arithmetic run on the CPU."""

    def __init__(self, plan):
        self.plan, self.z_dim = plan, plan["z_dim"]

    def intermediate(self, z):
        return torch.from_numpy(gr.intermediate(self.plan, z.numpy()).astype(np.float32))

    def forward(self, z):
        return torch.from_numpy(gr.run_plan(self.plan, torch.as_tensor(z).numpy()).astype(np.float32))


@pytest.mark.parametrize("name", VARIANTS)
def test_seeded_wrapper_draws_in_reference_order(name, tmp_path):
    path, ck = _checkpoint(name, tmp_path)
    w = object.__new__(controllable.GanWrapper)

    def load(p):
        w.generator = w.wgan = _PlanGenerator(gan.pack_generator(ck["generator_state_dict"], ck["model_parameters"]))
        w.mean, w.std = ck["dataset_mean"], ck["dataset_std"]

    w.load_model = load
    torch.manual_seed(int(G[f"{name}/wrapper_seed"]))
    controllable.GanWrapper.__init__(w, path, "cpu", controllability_samples=int(G["n_ctrl_samples"]))
    assert torch.equal(torch.cat(w.z_list[:4]), torch.from_numpy(G[f"{name}/z_head"]))
    assert torch.equal(torch.cat([w.z_list[s] for s in G["seeds"]]), torch.from_numpy(G[f"{name}/z_seeds"]))
    assert w.z is w.z_list[0] and w.normalize is False
    U = G[f"{name}/U"]
    assert np.abs(w.U.solution.numpy() - U).max() <= 1e-3 * np.abs(U).max()
    ref = G[f"{name}/modified"]
    w.set_latent(int(G["seeds"][2]))
    e = w.modify_embed(torch.from_numpy(G["sliders"][1]))
    assert np.abs(e.numpy()[0] - ref[2, 1]).max() <= 1e-4 * np.abs(ref).max()
    many = w.embeddings(seeds=[int(s) for s in G["seeds"]], controls=G["sliders"][1])
    assert torch.equal(many[2], e[0])


def test_no_cpu_path():
    with pytest.raises(capi.ToucanHipError):
        controllable.ControllableInterface(gpu_id="cpu")
    g, _ = fw.gan_state_dicts(dict(fw.GAN_PARAMS, size=4, nfilter=4, nfilter_max=8), 1)
    with pytest.raises(capi.ToucanHipError):
        gan.GeneratorEngine(g, dict(fw.GAN_PARAMS, size=4, nfilter=4, nfilter_max=8), "cpu")


def test_header_matches_binding():
    with open(os.path.join(REPO, "include", "toucan_gan.h")) as f:
        text = f.read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(re.findall(r"^int\s+(tts_\w+)\s*\(", body, flags=re.M))
    assert declared == sorted(capi.GAN_PROTOTYPES)
    consts = {k: int(v) for k, v in re.findall(r"#define TTS_GAN_(\w+) (\d+)", text)}
    assert (consts["KC"], consts["NC"]) == (capi.GAN_KC, capi.GAN_NC)
    assert [consts[k] for k in ("UPSAMPLE", "PRE_LRELU", "RESIDUAL", "RES_UPSAMPLE", "LRELU")] == \
        [capi.GAN_UPSAMPLE, capi.GAN_PRE_LRELU, capi.GAN_RESIDUAL, capi.GAN_RES_UPSAMPLE, capi.GAN_LRELU]
    struct = re.search(r"typedef struct TtsGanConvDesc \{(.*?)\} TtsGanConvDesc;", body, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*[,;]", struct)
    assert fields == [f for f, _ in capi.TtsGanConvDesc._fields_]
