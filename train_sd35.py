#!/usr/bin/env python3
"""SD3.5 trainer entry point -- same CLI as the reference (`train_sd35.py --config config.yaml`, train_sd35.py:196-204),
driving the MI355X-native MMDiT path (BASELINE config 4).

    python train_sd35.py --config config.yaml
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_sd35.py --config config.yaml

``pretrained_model_path`` (or ``pretrained_pipe_path``/transformer) must be a LOCAL diffusers directory; with neither the
SD3.5-Medium architecture is random-initialised (no network here).  The ``extract_features`` loop is outside the hot-path
scope: training consumes cached-feature shards whose samples carry the prompt embeddings (``emb.pt`` [333, 4096]) and the
pooled projection (``pooled.pt`` [2048]); ``python -m yat_amd.extract_latents`` makes their latents on the HIP AutoencoderKL
encoder (yat_amd/autoencoder_kl_encoder.py), which ``extract_latents`` also uses, and ``python -m yat_amd.encode_prompts`` makes
``emb.pt`` and ``pooled.pt`` on the HIP CLIP-L, OpenCLIP bigG and T5 encoders (yat_amd/clip.py, yat_amd/t5.py), which
``extract_embeddings`` also uses.  With ``<pretrained_pipe_path>/text_encoder{,_2,_3}`` + ``/tokenizer{,_2,_3}`` present, CFG
dropout needs no ``empty_embeds.pt`` and validation no ``validation_embeds.pt``; without them both come from those cached
files.  Validation decodes its latents on the HIP AutoencoderKL decoder (yat_amd/autoencoder_kl.py) when
``<pretrained_pipe_path>/vae`` holds the VAE.  The reference feeds the two CLIP encoders ``compress_caption(caption)`` (spaCy
plus a downloaded model, :79-92); that is not restated: CLIP gets the caption itself unless ``encode_prompts`` is given the
CLIP text separately.

Reference quirks: ``SD35Trainer.optimize(self, model, batch)`` (:165) has a pre-refactor signature with a
``(latents, embeddings, pooled_projections)`` batch no sampler produces any more, while ``Model.run`` calls
``optimize(ratio, latents, embeddings, repa_features, generator)`` (common/trainer.py:337) -- at HEAD the reference's SD3.5
entry raises TypeError on the first step; ``initialize`` (:160-163) refers to undefined names.  Here the recipe body is the
one written at :165-194 under the trainer's signature, with ``embeddings`` = the sampler's list of (prompt_embeds, pooled)
pairs.  Like the reference, noise and timestep draws come from the GLOBAL RNGs (:180,182), not the trainer's generator.
"""
import torch

from yat_amd import sampler
from yat_amd.common.aspect_ratios import ASPECT_RATIO_1024_BIN
from yat_amd.dit_trainer import DiTTrainer, main
from yat_amd.recipe import SD3Recipe
from yat_amd.scheduler import FlowMatchSchedule
from yat_amd.sd3 import SD3Config, SD3Transformer2DModelHIP


class SD35Trainer(DiTTrainer):
    """``extract_latents`` is train_sd35.py:63-77 on the HIP AutoencoderKL encoder (yat_amd/autoencoder_kl_encoder.py):
    ``(vae.encode(images).latent_dist.sample() - shift_factor) * scaling_factor``; the sample's noise comes from the device's
    global generator, as there.  The reference passes the images through ``image_processor.preprocess`` first (:68); for the
    fetcher's [-1, 1] tensors at bucket sizes that is taken to be the identity and is not restated here.  ``validate`` is
    :94-162: flow-match Euler sampling over the HIP MMDiT (:129-142), a CPU generator seeded 42 (:110), entries
    (prompt_embeds [1,T,C], negative_prompt_embeds, pooled_prompt_embeds [1,P], negative_pooled_prompt_embeds) (:116-118);
    the decode is :150-156.  ``extract_embeddings`` is :79-92 and the prompt encoding of ``validate`` :113-118 on the three HIP
    text encoders (yat_amd/clip.py, yat_amd/t5.py, yat_amd/encode_prompts.py), built at the first call from
    ``<pretrained_pipe_path>/text_encoder{,_2,_3}`` + ``/tokenizer{,_2,_3}``; it returns one (prompt_embeds [333, J], pooled [P])
    pair per caption.  As in the reference the decoder's argument is ``latent / scaling_factor`` WITHOUT
    ``+ shift_factor`` (:155; diffusers' own SD3 pipeline adds it): this keeps the reference's outward contract
    (yat_amd/autoencoder_kl.py ``pre_scale``).  ``optimize`` is :165-194 (``SD3Recipe``); global RNG streams as there."""
    model_cls, config_cls, recipe_cls = SD3Transformer2DModelHIP, SD3Config, SD3Recipe              # :28-43
    aspect_ratios = ASPECT_RATIO_1024_BIN                                                           # :55
    apply_shift = True
    validation_seed_on_device = False
    text_encoder_kind, text_encoder_noun = "clip_text_model", "CLIP-L + OpenCLIP bigG + T5 (text_encoder, _2, _3)"   # :79-92, :113-118

    def make_scheduler(self, raw):
        return FlowMatchSchedule(shift=float(raw.get("shift", 3.0)))                                # :49

    def sample_validation(self, embeds, side, generator):
        pe, ne, pp, npp = embeds
        return sampler.sample_latents_sd3(self.model, pe, pp, ne, npp, side, side, num_inference_steps=20, guidance_scale=5.0,
                                          generator=generator, schedule=self.scheduler)

    def check_text_encoder_width(self, encoder):
        """``SD3Config`` has no ``caption_channels``: a prompt row enters at ``joint_attention_dim``, the pooled vector at
        ``pooled_projection_dim``."""
        cfg = self.model.config
        if encoder.H != cfg.joint_attention_dim or encoder.pooled_dim != cfg.pooled_projection_dim:
            raise ValueError(f"the text encoders give prompt rows of width {encoder.H} and a pooled vector of {encoder.pooled_dim}; "
                             f"the transformer's joint_attention_dim is {cfg.joint_attention_dim} and its pooled_projection_dim "
                             f"{cfg.pooled_projection_dim}")

    def check_empty_embeddings(self, emb, path):
        """SD3.5's per-sample embedding is a ``(prompt_embeds [T, C], pooled [P])`` pair (``SD3Recipe.stack_embeddings``), so
        ``empty_embeds.pt`` holds that pair for the empty prompt -- as the pair itself or as a list with the pair (what
        ``extract_embeddings([''])`` returns, :76-92).  A bare tensor (the SANA / PixArt layout) is an error here: CFG
        dropout would slice it by rows."""
        if isinstance(emb, (list, tuple)) and len(emb) == 1 and isinstance(emb[0], (list, tuple)):
            emb = emb[0]
        ok = (isinstance(emb, (list, tuple)) and len(emb) == 2 and all(torch.is_tensor(t) for t in emb)
              and emb[0].ndim in (2, 3) and emb[1].numel() == emb[1].shape[-1])
        if not ok:
            raise ValueError(f"{path}: SD3.5 needs the empty prompt's (prompt_embeds [T, C], pooled [P]) pair, got "
                             f"{type(emb).__name__}" + (f" of shape {tuple(emb.shape)}" if torch.is_tensor(emb) else ""))
        prompt = emb[0] if emb[0].ndim == 2 else emb[0][0]
        return [(prompt, emb[1].reshape(-1))]


if __name__ == "__main__":
    main(SD35Trainer, "extract_features needs the R2 transport, which is outside this build's scope; `python -m "
                      "yat_amd.extract_latents` and `python -m yat_amd.encode_prompts` make the cached features")
