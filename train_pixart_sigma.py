#!/usr/bin/env python3
"""PixArt-Sigma trainer entry point -- same CLI as the reference (`train_pixart_sigma.py --config config.yaml`,
train_pixart_sigma.py:187-198), driving the MI355X-native path (BASELINE config 3).

    python train_pixart_sigma.py --config config.yaml
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_pixart_sigma.py --config config.yaml

``pretrained_model_path`` (or ``pretrained_pipe_path``/transformer) must be a LOCAL diffusers directory; with neither the
PixArt-Sigma-XL-2 architecture is random-initialised (no network here).  The ``extract_features`` loop is outside the
hot-path scope: training consumes cached-feature shards (``python -m yat_amd.extract_latents`` makes their latents on the HIP
AutoencoderKL encoder, which ``extract_latents`` also uses; ``python -m yat_amd.encode_prompts`` makes their prompt embeddings
on the HIP T5 encoder, which ``extract_embeddings`` also uses).  With ``<pretrained_pipe_path>/text_encoder`` + ``/tokenizer``
present, CFG dropout needs no ``empty_embeds.pt`` and validation no ``validation_embeds.pt``; without them both come from
those cached files.  When ``<pretrained_pipe_path>/vae`` holds the AutoencoderKL, validation decodes its latents to images on
the HIP decoder (yat_amd/autoencoder_kl.py).

Reference quirk: ``PixartSigmaTrainer.optimize(self, latents, embeddings)`` (:151) still has the two-argument signature
while ``Model.run`` calls ``optimize(ratio, latents, embeddings, repa_features, generator)`` (common/trainer.py:337) -- at
HEAD the reference's PixArt entry point raises TypeError on the first step.  Here the recipe body is the one written at
:151-185 and the signature is the trainer's.
"""
from yat_amd import sampler
from yat_amd.dit_trainer import DiTTrainer, main
from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
from yat_amd.recipe import PixArtRecipe
from yat_amd.scheduler import DDPMSchedule


class PixartSigmaTrainer(DiTTrainer):
    """``extract_latents`` is train_pixart_sigma.py:61-66 on the HIP AutoencoderKL encoder (yat_amd/autoencoder_kl_encoder.py):
    ``vae.encode(images).latent_dist.sample() * scaling_factor``, never a shift; the sample's noise comes from the device's
    global generator, as there.  ``validate`` is :76-149: DPM-Solver++ sampling (:117-129; ``pag_scale`` lands in the plain
    pipeline's ``**kwargs`` and is ignored), generator seeded 42 on the device (:94), entries (prompt_embeds [1,T,C], mask
    [1,T], negative_embeds, negative_mask) (:100-108); the decode is :137-144.  ``optimize`` is :151-185 (``PixArtRecipe``):
    the reference draws noise and timesteps from the GLOBAL RNGs (:170,172) and ignores the trainer's per-step generator; so
    does this.  ``extract_embeddings`` is :68-74 and the prompt encoding of ``validate`` :97-108 on the HIP T5 encoder
    (yat_amd/t5.py, yat_amd/encode_prompts.py), built at the first call from ``<pretrained_pipe_path>/text_encoder`` +
    ``/tokenizer``."""
    model_cls, config_cls, recipe_cls = PixArtTransformer2DModelHIP, PixArtConfig, PixArtRecipe     # :24-33
    recipe_args = {"pad_to": 300}
    vae_compression, apply_shift = 8, False                                                         # :41-50
    text_encoder_kind, text_encoder_noun = "t5", "T5"                                               # :68-74, :97-108

    def __init__(self, params, accelerator=None, config: PixArtConfig | None = None):
        if getattr(params, "use_repa", False):
            # REPAPixArtTransformerModel (:26,31) only adds a projector whose output never reaches the loss
            # (common/trainer.py:340-341 is commented out): nothing to train there
            print("[Warning] use_repa: the REPA projector is not built (its loss term is disabled in the reference)")
        super().__init__(params, accelerator, config)

    def make_scheduler(self, raw):                                                                  # :37
        if raw.get("beta_schedule", "linear") != "linear":
            raise NotImplementedError(f"beta_schedule {raw['beta_schedule']!r}")
        return DDPMSchedule(**{k: raw[k] for k in ("num_train_timesteps", "beta_start", "beta_end") if k in raw})

    def sample_validation(self, embeds, side, generator):
        pe, pm, ne, nm = embeds
        return sampler.sample_latents_pixart(self.model, pe, pm, ne, nm, side, side, num_inference_steps=20, guidance_scale=5.0,
                                             generator=generator)


if __name__ == "__main__":
    main(PixartSigmaTrainer, "extract_features needs the R2 transport, which is outside this build's scope; `python -m "
                             "yat_amd.extract_latents` and `python -m yat_amd.encode_prompts` make the cached features")
