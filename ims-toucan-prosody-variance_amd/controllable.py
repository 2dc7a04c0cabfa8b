"""Drop-in counterparts of the reference's artificial-voice front end on the HIP kernels:

* ``GanWrapper`` - InferenceInterfaces/Controllability/GAN.py:8-81: the same constructor, attributes (``U``, ``z_list``, ``z``,
  ``mean``, ``std``, ``normalize``, ``device``) and methods, with the generator ResNet_G on the GPU (gan.GeneratorEngine).
  Additive: ``embeddings(seeds, controls, latents)`` - many voices in one generator pass - and the constructor keyword
  ``controllability_samples`` (the reference's fixed 50 000).
* ``ControllableInterface`` - InferenceInterfaces/ControllableInterface.py:10-124: the same constructor and ``read``, plus the
  additive keyword ``input_is_phones``.

Random draws come from torch's CPU generator in the reference's order - the latents of ``compute_controllability``, the random
basis of ``torch.pca_lowrank``, then the 1100 voices of ``z_list`` - so a seeded construction gives the reference's ``U`` and
``z_list``.  Stated deviations: fp32 only; ``compute_controllability`` runs only the generator's first layer
(all that the reference uses of its pass); no gradio GUI; no grapheme-to-phoneme conversion (raw text raises, as in
ToucanTTSInterface; phoneme strings go through ``input_is_phones=True``).
"""
import os

import numpy as np
import torch

from . import capi, gan, interface

Z_DIM = 32  # GAN.py:22 and :28 draw 32-dimensional latents
N_VOICES = 1100  # GAN.py:21


def inverse_normalize(tensor, mean, std):
    return tensor * std + mean


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise capi.ToucanHipError(f"device {device!r}: the speaker-embedding GAN runs on the GPU only (no CPU path)")
    return dev


class GanWrapper:

    def __init__(self, path_wgan, device, controllability_samples=50000):
        self.device = device
        self.path_wgan = path_wgan

        self.mean = None
        self.std = None
        self.wgan = None
        self.normalize = False

        self.load_model(path_wgan)

        self.U = self.compute_controllability(n_samples=controllability_samples)
        self.z_list = list()
        for _ in range(N_VOICES):
            self.z_list.append(torch.randn((1, Z_DIM)))  # ResNet_G.sample_latent(1, 32) (resnet_1.py:79-80)
        self.z = self.z_list[0]

    def set_latent(self, seed):
        self.z = self.z_list[seed]

    def reset_default_latent(self):
        self.z = torch.randn((1, Z_DIM))

    def load_model(self, path):
        gan_checkpoint = torch.load(path, map_location="cpu", weights_only=True)
        # the generator only: the critic (ResNet_D) is loaded by the reference but never run at inference
        self.generator = gan.GeneratorEngine(gan_checkpoint["generator_state_dict"], gan_checkpoint["model_parameters"], _device(self.device))
        self.wgan = self.generator  # (the reference's attribute; here the engine itself)
        self.mean = gan_checkpoint["dataset_mean"]
        self.std = gan_checkpoint["dataset_std"]

    def compute_controllability(self, n_samples=50000):
        # The reference's sample_generator (wgan_qc.py:238-253) runs the whole generator on all n_samples latents and throws the
        # images away: only l_1, the output of fc -> BatchNorm1d -> LeakyReLU, is used.  So only that first layer runs here.
        z = torch.randn((n_samples, self.generator.z_dim))  # CPU generator, as sample_latent
        intermediate = self.generator.intermediate(z).cpu()
        return self.controllable_speakers(intermediate, z)

    def controllable_speakers(self, intermediate, z):
        pca = torch.pca_lowrank(intermediate)
        mu = intermediate.mean()  # one scalar over the whole matrix, as the reference
        X = torch.matmul((intermediate - mu), pca[2])
        U = torch.linalg.lstsq(X, z)
        return U

    def _finish(self, embed):
        if self.normalize:
            embed = inverse_normalize(embed.cpu(), self.mean.cpu().unsqueeze(0), self.std.cpu().unsqueeze(0))
        return embed

    def get_original_embed(self):
        return self._finish(self.generator.forward(self.z))

    def _modified_latent(self, z, x):
        return z.squeeze() + torch.matmul(self.U.solution.t(), x)

    def modify_embed(self, x):
        z_new = self._modified_latent(self.z, x)
        return self._finish(self.generator.forward(z_new.unsqueeze(0)))

    def embeddings(self, seeds=None, controls=None, latents=None):
        """Many voices in one generator pass: [N, data_dim] on the device.  ``latents`` [N, 32], or ``seeds`` (indices into
        ``z_list``; default the current voice), each moved by its row of ``controls`` [N, 6] (or one [6] vector for all) as
        ``modify_embed`` moves it.  Row i equals ``modify_embed`` of the same voice and sliders bit for bit."""
        if latents is not None:
            if seeds is not None:
                raise ValueError("give seeds or latents, not both")
            zs = [z.reshape(1, -1) for z in torch.as_tensor(latents, dtype=torch.float32)]
        else:
            zs = [self.z] if seeds is None else [self.z_list[int(s)] for s in np.atleast_1d(seeds)]
        if controls is not None:
            controls = torch.as_tensor(controls, dtype=torch.float32)
            if controls.dim() == 1:
                controls = controls.expand(len(zs), -1)
            if controls.shape[0] != len(zs):
                raise ValueError(f"{controls.shape[0]} control vectors for {len(zs)} voices")
            # per voice, the same CPU arithmetic as modify_embed
            zs = [self._modified_latent(z, c).reshape(1, -1) for z, c in zip(zs, controls)]
        return self._finish(self.generator.forward(torch.cat(zs)))


_TOO_LONG = "Your input was too long. Please try either a shorter text or split it into several parts."


class ControllableInterface:

    def __init__(self, gpu_id="cpu", available_artificial_voices=1000):
        if gpu_id == "cpu":
            raise capi.ToucanHipError("ControllableInterface(gpu_id='cpu'): the HIP kernels have no CPU path; pass a GPU index")
        # the reference selects the GPU through CUDA_VISIBLE_DEVICES and then uses "cuda"; here the index selects the device directly
        self.device = f"cuda:{int(gpu_id)}"
        self.model = interface.ToucanTTSInterface(device=self.device, tts_model_path="Meta")
        self.wgan = GanWrapper(os.path.join(interface.MODELS_DIR, "Embedding", "embedding_gan.pt"), device=self.device)
        self.generated_speaker_embeds = list()
        self.available_artificial_voices = available_artificial_voices
        self.current_language = "English"
        self.current_accent = "English"
        self.language_id_lookup = {
            "English"   : "en",
            "German"    : "de",
            "Greek"     : "el",
            "Spanish"   : "es",
            "Finnish"   : "fi",
            "Russian"   : "ru",
            "Hungarian" : "hu",
            "Dutch"     : "nl",
            "French"    : "fr",
            'Polish'    : "pl",
            'Portuguese': "pt",
            'Italian'   : "it",
            'Chinese'   : "cmn",
            'Vietnamese': "vi",
        }

    def read(self, prompt, language, accent, voice_seed, duration_scaling_factor, pause_duration_scaling_factor, pitch_variance_scale,
             energy_variance_scale, emb_slider_1, emb_slider_2, emb_slider_3, emb_slider_4, emb_slider_5, emb_slider_6,
             input_is_phones=False):
        """ControllableInterface.py:42-124: (48000, the wave with every sample doubled, the path of the plot).  The voice is
        ``z_list[voice_seed]`` moved by the six sliders.  ``input_is_phones=True`` takes ``prompt`` as a phoneme string; a prompt
        of more than 1800 phonemes raises ValueError (the reference reads an apology in the chosen language instead, which would
        need grapheme-to-phoneme conversion)."""
        language = language.split()[0]
        accent = accent.split()[0]
        if self.current_language != language:
            self.model.set_phonemizer_language(self.language_id_lookup[language])
            self.current_language = language
        if self.current_accent != accent:
            self.model.set_accent_language(self.language_id_lookup[accent])
            self.current_accent = accent

        self.wgan.set_latent(voice_seed)
        controllability_vector = torch.tensor([emb_slider_1, emb_slider_2, emb_slider_3, emb_slider_4, emb_slider_5, emb_slider_6],
                                              dtype=torch.float32)
        embedding = self.wgan.modify_embed(controllability_vector)
        self.model.set_utterance_embedding(embedding=embedding)

        phones = prompt if input_is_phones else self.model.text2phone.get_phone_string(prompt)
        if len(phones) > 1800:
            raise ValueError(f"{len(phones)} phonemes: {_TOO_LONG}")

        wav, fig = self.model(prompt, input_is_phones=input_is_phones, duration_scaling_factor=duration_scaling_factor,
                              pitch_variance_scale=pitch_variance_scale, energy_variance_scale=energy_variance_scale,
                              pause_duration_scaling_factor=pause_duration_scaling_factor, return_plot_as_filepath=True)
        wav = wav.cpu().numpy()
        wav = [val for val in wav for _ in (0, 1)]  # doubling the sampling rate for better compatibility (24kHz is not as standard as 48kHz)
        return 48000, wav, fig
