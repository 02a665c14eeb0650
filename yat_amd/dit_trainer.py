"""What the three DiT entry points (train_sana.py, train_pixart_sigma.py, train_sd35.py) share: the transformer lookup with
its random-init fallback, the scheduler config read, the VAE bookkeeping, ``extract_latents`` / ``extract_embeddings``,
``validate`` and the fast-path ``optimize``.  An entry point states its model's facts as class attributes and two small
overrides (``make_scheduler``, ``sample_validation``); its docstring carries the reference citations."""
import argparse
import json
import os

import torch

from .autoencoder_kl import load_vae_decoder, load_vae_encoder
from .common.aspect_ratios import table_for_resolution
from .common.trainer import Model
from .common.training_parameters_reader import TrainingParameters
from .vae_common import decode_validation, find_vae_dir


class DiTTrainer(Model):
    model_cls = config_cls = recipe_cls = None
    recipe_args = {}                # beside (model, scheduler, device=...)
    vae_compression = None          # latent -> pixel factor that picks the aspect table; None: ``aspect_ratios`` is set
    vae_noun = "AutoencoderKL"
    apply_shift = None              # ``encode(images, apply_shift=...)``; None: the encoder takes no such argument (DC-AE)
    validation_seed_on_device = True
    step_generator = False          # hand the trainer's per-step generator to the recipe (else: the global RNG streams)
    text_encoder_kind = None        # "gemma2" / "t5" / "clip_text_model": the pipe's text encoder, built at first use (yat_amd/encode_prompts.py);
    text_encoder_noun = None        # None: this trainer has no text side and trains from cached embeddings only

    def __init__(self, params: TrainingParameters, accelerator=None, config=None):
        super().__init__(params, accelerator)
        dev = self.accelerator.device
        path = params.pretrained_model_path
        if path is None and params.pretrained_pipe_path and os.path.isdir(os.path.join(params.pretrained_pipe_path, "transformer")):
            path = os.path.join(params.pretrained_pipe_path, "transformer")
        if path is not None and os.path.isdir(path):
            self.model = self.model_cls.from_pretrained(path, device=dev)
        else:
            self.model = self.model_cls(config or self.config_cls(), device=dev).init_synthetic(0)
        self.model.enable_gradient_checkpointing()                                             # (no-op here)
        raw = {}
        sched_cfg = os.path.join(params.pretrained_pipe_path or "", "scheduler", "scheduler_config.json")
        if os.path.isfile(sched_cfg):
            with open(sched_cfg) as f:
                raw = json.load(f)
        self.scheduler = self.make_scheduler(raw)
        if self.vae_compression is not None:
            self.aspect_ratios = table_for_resolution(self.model.config.sample_size * self.vae_compression)
        self.recipe = self.recipe_cls(self.model, self.scheduler, device=dev, **self.recipe_args)
        self.pipe = None
        self.vae_dir = find_vae_dir(params.pretrained_pipe_path)
        self.vae = None                                                                        # built at the first validate()
        self.vae_encoder = None                                                                # built at the first extract_latents()

    def make_scheduler(self, raw):
        """``raw``: the pipe's ``scheduler/scheduler_config.json``, {} without one."""
        raise NotImplementedError

    def sample_validation(self, embeds, side, generator):
        """One entry of ``validation_embeds.pt`` -> latents, through the model's sampler in ``yat_amd.sampler``."""
        raise NotImplementedError

    def _vae_encoder(self):
        """The VAE encoder, built once; NotImplementedError without ``<pretrained_pipe_path>/vae``."""
        self._require_vae()
        if self.vae_encoder is None:
            self.vae_encoder = load_vae_encoder(self.vae_dir, device=self.accelerator.device)
        return self.vae_encoder

    def _require_vae(self):
        if self.vae_dir is None:
            want = os.path.join(self.params.pretrained_pipe_path or "<pretrained_pipe_path>", "vae")
            raise NotImplementedError(f"VAE encoding needs the {self.vae_noun} in {want!r} (config.json + safetensors); without "
                                      "it, train from cached-feature shards")

    def extract_latents(self, images):
        enc = self._vae_encoder()
        if self.apply_shift is None:
            return enc.encode(images)
        return enc.encode(images, apply_shift=self.apply_shift)

    def extract_latents_uint8(self, images_u8, generator=None):
        """``[B, H, W, 3]`` uint8 -> what ``extract_latents`` gives for ToTensor -> Normalize(0.5, 0.5) of them; an AutoencoderKL
        draws its sample's noise from ``generator``."""
        enc = self._vae_encoder()
        if self.apply_shift is None:
            return enc.encode_uint8(images_u8)
        return enc.encode_uint8(images_u8, apply_shift=self.apply_shift, generator=generator)

    def check_feature_extractors(self):
        self._require_vae()
        self._require_text_dirs()

    def _text_encoder(self):
        """(encoder, tokenizer), built once from ``<pretrained_pipe_path>/text_encoder`` + ``/tokenizer``;
        NotImplementedError without the two directories (raised before the model or the device is looked at)."""
        if self.text_encoder_kind is None:
            raise NotImplementedError("text encoding is outside the hot-path scope; train from cached-feature shards")
        from .encode_prompts import load_encoder
        enc = getattr(self, "text_encoder", None)
        if enc is not None and enc[0].layers is not None:
            return enc
        pipe = self._require_text_dirs()
        enc = load_encoder(pipe, device=self.accelerator.device)
        self.check_text_encoder_width(enc[0])
        print(enc[0].describe())
        self.text_encoder = enc
        return enc

    def _require_text_dirs(self):
        """-> the pipe directory; NotImplementedError without its text encoder and tokenizer directories."""
        if self.text_encoder_kind is None:
            raise NotImplementedError("text encoding is outside the hot-path scope; train from cached-feature shards")
        from .encode_prompts import find_text_dirs
        pipe = getattr(self.params, "pretrained_pipe_path", None)
        if find_text_dirs(pipe, self.text_encoder_kind) is None:
            want = os.path.join(pipe or "<pretrained_pipe_path>", "text_encoder")
            raise NotImplementedError(f"text encoding needs the {self.text_encoder_noun} encoder in {want!r} (config.json + "
                                      "safetensors) and the tokenizer beside it; without them text encoding is outside the hot-path "
                                      "scope: train from cached-feature shards")
        return pipe

    def check_text_encoder_width(self, encoder):
        """ValueError when the encoder's rows do not fit the transformer."""
        want = self.model.config.caption_channels
        if encoder.H != want:
            raise ValueError(f"the text encoder's hidden size {encoder.H} is not the transformer's caption_channels {want}")

    def extract_embeddings(self, captions):
        from .encode_prompts import extract_embeddings
        encoder, tokenizer = self._text_encoder()
        return extract_embeddings(encoder, tokenizer, captions, max_batch=getattr(self.params, "text_encoder_max_batch_size", None))

    def load_empty_embeddings(self):
        emb = super().load_empty_embeddings()
        if self.text_encoder_kind is None:
            return emb
        # the step stages its embeddings from the host (SD3.5: a (prompt, pooled) pair per sample)
        return [tuple(t.cpu() for t in e) if isinstance(e, (tuple, list)) else e.cpu() for e in emb]

    def encode_validation_prompts(self):
        """The first third of the reference's ``validate()`` for a trainer that has a text encoder: the entries of
        ``validation_embeds.pt`` made from ``params.validation_prompts``, encoded once and kept for the later validations;
        the encoder's weights are freed afterwards, unless ``compute_features`` keeps encoding captions with it.  None without
        a text encoder."""
        kept = getattr(self, "validation_embeds", None)
        if kept is not None:
            return kept
        try:
            encoder, tokenizer = self._text_encoder()
        except NotImplementedError:
            return None
        from .encode_prompts import validation_embeddings
        self.validation_embeds = validation_embeddings(encoder, tokenizer, list(self.params.validation_prompts or []))
        if not getattr(self.params, "compute_features", None):     # (the extract-features sampler encodes every batch with it)
            encoder.free()
            self.text_encoder = None
        return self.validation_embeds

    def validate(self):
        """The middle third of the reference's ``validate()``: 20 sampling steps with CFG 5.0 over the HIP transformer,
        generator seeded 42.  The prompt embeddings come from a cached file (``validation_embeds.pt`` next to the shards or in
        the cwd: a list of tuples as ``pipe.encode_prompt`` returns them) or, without one, from ``encode_validation_prompts``
        (with the text encoders in the pipe directory: SANA's Gemma-2, PixArt-Sigma's T5, SD3.5's CLIP-L + OpenCLIP bigG + T5),
        and the result is the latents (``output_type='latent'``), stored under models/<step>/ with a three-channel
        preview for the logger.  With a VAE in ``<pretrained_pipe_path>/vae`` the last third runs too: each latent is decoded
        on the HIP decoder (built at the first call; ``vae.decode(latent / scaling_factor)`` -> ``postprocess``), logged as
        ``validation/{idx}/{prompt}`` and written to models/<step>/validation_{idx}.png."""
        cands = [os.path.join(os.path.dirname(p), "validation_embeds.pt") for p in (self.params.local_shard_paths or [])]
        path = next((c for c in cands + ["validation_embeds.pt"] if os.path.isfile(c)), None)
        embeds = torch.load(path, map_location="cpu") if path is not None else self.encode_validation_prompts()
        if embeds is None:
            raise NotImplementedError("no cached validation embeddings (text encoding is outside the hot-path scope)")
        gen = torch.Generator(device=self.accelerator.device if self.validation_seed_on_device else "cpu").manual_seed(42)
        side = self.model.config.sample_size
        out = [self.sample_validation(e, side, gen).cpu() for e in embeds]
        os.makedirs(f"models/{self.global_step}", exist_ok=True)
        torch.save(out, f"models/{self.global_step}/validation_latents.pt")
        if self.logger is not None:                # the reference logs the decoded image; without the VAE: a latent preview
            for idx, lat in enumerate(out):
                x = lat[0, :3].float()
                x = (x - x.amin()) / (x.amax() - x.amin()).clamp_min(1e-6)
                self.logger.add_image(f"validation_latents/{idx}", x, self.global_step)
        if self.vae_dir is not None:
            if self.vae is None:
                self.vae = load_vae_decoder(self.vae_dir, device=self.accelerator.device)
            decode_validation(self.vae, out, self.params.validation_prompts, self.global_step, self.logger)
        return out

    def optimize(self, ratio, latents, embeddings, repa_tokens=None, generator: torch.Generator = None):
        """With gradients enabled (the training call, common/trainer.py:337) the step runs on the allocation-free device path
        -- one packed H2D copy, forward, loss and backward as straight-line launches replayed from launch plans (the recipe's
        ``optimize_device``) -- and the returned loss is marked so that ``accelerator.backward`` does not run a second
        backward; under ``no_grad`` (exploration trials, :326-336) it is the plain forward + loss."""
        generator = generator if self.step_generator else None
        if torch.is_grad_enabled() and not latents.is_cuda and os.environ.get("YAT_TRAINER_FAST", "1") != "0":
            loss = self.recipe.optimize_device(latents, embeddings, generator,
                                               gscale=1.0 / self.accelerator.gradient_accumulation_steps)
            loss.yat_backward_done = True
            return loss
        return self.recipe.optimize(latents, embeddings, generator)


def main(trainer_cls, extract_features_message):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", required=True, type=str)
    parser.add_argument("--max-steps", type=int, default=None)
    args = parser.parse_args()
    params = TrainingParameters()
    params.read_yaml(args.config)
    if params.extract_features:
        raise SystemExit(extract_features_message)
    trainer_cls(params).run(max_steps=args.max_steps)
