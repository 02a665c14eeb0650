#!/usr/bin/env python3
"""SANA trainer entry point -- same CLI as the reference (`train_sana.py --config config.yaml`, README.md:45,
train_sana.py:221-237), driving the MI355X-native hot path.

    python train_sana.py --config config.yaml                      # 1 GPU
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_sana.py --config config.yaml

``pretrained_model_path`` (or ``pretrained_pipe_path``/transformer) must be a LOCAL diffusers directory
(config.json + diffusion_pytorch_model.safetensors); with neither present the 1.6B architecture is random-initialised
(there is no network here).  Training consumes cached-feature shards (``python -m yat_amd.extract_latents`` makes their
latents on the HIP DC-AE encoder, which ``extract_latents`` also uses; ``python -m yat_amd.encode_prompts`` makes their prompt
embeddings on the HIP Gemma-2 encoder, which ``extract_embeddings`` also uses) or, with ``compute_features: true`` (plus
``vae_max_batch_size`` / ``text_encoder_max_batch_size``) and ``<pretrained_pipe_path>/vae`` + ``/text_encoder`` +
``/tokenizer`` present, raw WebDataset shards of ``*.jpg`` + ``*.txt`` as img2dataset writes them: each image is resized
to its bucket by the Pillow-exact HIP resize and encoded on the fly (``BucketSamplerExtractFeatures``).  The
``extract_features`` loop (R2 upload) is outside the hot-path scope.  With ``<pretrained_pipe_path>/text_encoder`` + ``/tokenizer`` present, CFG dropout
needs no ``empty_embeds.pt`` and validation no ``validation_embeds.pt``; without them both come from those cached files.
When ``<pretrained_pipe_path>/vae`` holds the DC-AE, validation decodes its latents to images on the HIP decoder
(yat_amd/dcae.py).
"""
from yat_amd import sampler
from yat_amd.dit_trainer import DiTTrainer, main
from yat_amd.recipe import SanaRecipe
from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
from yat_amd.scheduler import FlowMatchSchedule


class SanaModel(DiTTrainer):
    """``extract_latents`` is train_sana.py:78-82 on the HIP DC-AE encoder (yat_amd/dcae_encoder.py):
    ``vae.encode(images.to(bf16)).latent.to(bf16) * scaling_factor``.  ``validate`` is :99-161: flow-match Euler sampling,
    generator seeded 42 on the device (:108), entries (prompt_embeds [1,T,C], mask [1,T], negative_embeds, negative_mask);
    the decode on the HIP DC-AE decoder (yat_amd/dcae.py) is :153-157.  ``optimize`` is :163-219 with the trainer's per-step
    generator (``SanaRecipe``).  ``extract_embeddings`` is :84-94 and the prompt encoding of ``validate`` :113-129 on the HIP
    Gemma-2 encoder (yat_amd/gemma2.py, yat_amd/encode_prompts.py), built at the first call from
    ``<pretrained_pipe_path>/text_encoder`` + ``/tokenizer``."""
    model_cls, config_cls, recipe_cls = SanaTransformer2DModelHIP, SanaConfig, SanaRecipe           # train_sana.py:20-23
    recipe_args = {"pad_to": 512}
    vae_compression, vae_noun = 32, "DC-AE"                                                         # :45-57
    step_generator = True
    text_encoder_kind, text_encoder_noun = "gemma2", "Gemma-2"                                      # :84-94, :113-131

    def make_scheduler(self, raw):
        return FlowMatchSchedule(shift=float(raw.get("shift", 3.0)))                                # :41

    def sample_validation(self, embeds, side, generator):
        pe, pm, ne, nm = embeds
        return sampler.sample_latents(self.model, pe, pm, ne, nm, side, side, num_inference_steps=20, guidance_scale=5.0,
                                      generator=generator, schedule=self.scheduler)


if __name__ == "__main__":
    main(SanaModel, "extract_features needs the text encoder and the R2 transport, which are outside this build's scope; "
                    "`python -m yat_amd.extract_latents` encodes image files into a shard on the HIP DC-AE encoder")
