"""What the VAE halves on the HIP path share (yat_amd/dcae.py, yat_amd/dcae_encoder.py, yat_amd/autoencoder_kl.py,
yat_amd/autoencoder_kl_encoder.py): reading a diffusers ``vae`` directory, the strict state-dict check, the host side of a
``*HIP`` class, the uint8 postprocess, the trainers' validation-image loop and the latents -> PNG command line."""
from __future__ import annotations

import argparse
import json
import os

import torch

BF16 = torch.bfloat16


def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """torch [Cout, Cin, 3, 3] -> [Cout, 3, 3, Cin] (K = 9 Cin contiguous, tap-major)."""
    return w.permute(0, 2, 3, 1).contiguous()


def find_vae_dir(pretrained_pipe_path) -> str | None:
    """``<pipe>/vae`` when it holds a ``config.json`` (the VAE the trainers' validate() builds), else None."""
    if not pretrained_pipe_path:
        return None
    d = os.path.join(pretrained_pipe_path, "vae")
    return d if os.path.isfile(os.path.join(d, "config.json")) else None


def read_config(vae_dir: str) -> dict:
    with open(os.path.join(vae_dir, "config.json")) as f:
        return json.load(f)


def load_tensors(vae_dir: str, keep) -> dict:
    """The tensors of a diffusers VAE directory whose key ``keep`` accepts."""
    from safetensors import safe_open
    with safe_open(os.path.join(vae_dir, "diffusion_pytorch_model.safetensors"), framework="pt") as f:
        return {k: f.get_tensor(k) for k in f.keys() if keep(k)}


def check_expected(want: dict, sd: dict, ours, noun: str, consumer: str) -> None:
    """Strict load: every key of ``want`` ({key: shape}) present in ``sd`` with its shape, and no other key that ``ours``
    accepts.  Raises KeyError / ValueError naming the key; ``noun`` and ``consumer`` word the messages."""
    for k, shape in want.items():
        if k not in sd:
            raise KeyError(f"{noun} weight {k!r} is missing from the checkpoint")
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"{noun} weight {k!r} has shape {tuple(sd[k].shape)}, expected {shape}")
    extra = sorted(k for k in sd if ours(k) and k not in want)
    if extra:
        raise KeyError(f"{noun} weight {extra[0]!r} is not consumed by {consumer} ({len(extra)} unconsumed key(s))")


def to_uint8(images: torch.Tensor) -> torch.Tensor:
    """VaeImageProcessor.postprocess(output_type='pil') up to the PIL image: [B, 3, H, W] bf16 -> uint8 (CHW)."""
    from . import ops
    return ops.dcae_image_to_uint8(images.contiguous())


class VAEHalfHIP:
    """Host side of one VAE half in bf16 on the HIP kernels: the packed weights on the device and the activation buffers of
    the last size.  A subclass sets ``load_vae_dir`` (directory -> (cfg, tensors)) and ``pack_weights`` (cfg, tensors ->
    packed) as static methods and supplies ``_alloc_buffers(h, w)``."""

    def __init__(self, cfg, packed: dict, device="cuda"):
        self.cfg = cfg
        self.device = torch.device(device)
        self.w = {k: v.to(self.device, BF16).contiguous() for k, v in packed.items()}
        self._bufs = None

    @classmethod
    def from_pretrained(cls, vae_dir: str, device="cuda"):
        cfg, sd = cls.load_vae_dir(vae_dir)
        return cls(cfg, cls.pack_weights(cfg, sd), device)

    def _buffers(self, h, w):
        if self._bufs is not None and self._bufs[0] == (h, w):
            return self._bufs[1]
        self._bufs = None                                   # the old buffers go before the new ones come: bounds the peak
        bufs = self._alloc_buffers(h, w)
        self._bufs = ((h, w), bufs)
        return bufs

    to_uint8 = staticmethod(to_uint8)


def decode_validation(vae, latents, prompts, step, logger):
    """The last third of the trainers' ``validate()`` (train_sana.py:153-157, train_pixart_sigma.py:137-144,
    train_sd35.py:150-156): each latent decoded, written to models/<step>/validation_{idx}.png and logged as
    ``validation/{idx}/{prompt}``."""
    from .common.tb_writer import encode_png
    prompts = list(prompts or [])
    for idx, lat in enumerate(latents):
        img = vae.to_uint8(vae.decode(lat if lat.dim() == 4 else lat[None]))[0].cpu()
        with open(f"models/{step}/validation_{idx}.png", "wb") as f:
            f.write(encode_png(img))
        if logger is not None:
            tag = f"validation/{idx}/{prompts[idx]}" if idx < len(prompts) else f"validation/{idx}"
            logger.add_image(tag, img, step)


def latents_to_png_main(prog: str, noun: str, decoder_cls, argv=None) -> None:
    """The latents-file -> PNG command line of ``python -m yat_amd.dcae`` / ``yat_amd.autoencoder_kl``."""
    ap = argparse.ArgumentParser(prog=prog, description="decode a validation_latents.pt (list of [1, C, h, w]) into PNG files")
    ap.add_argument("--vae", required=True, help=f"diffusers {noun} directory (config.json + safetensors)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("latents")
    ap.add_argument("out_dir")
    a = ap.parse_args(argv)
    from .common.tb_writer import encode_png
    dec = decoder_cls.from_pretrained(a.vae, device=a.device)
    lats = torch.load(a.latents, map_location="cpu")
    if isinstance(lats, torch.Tensor):
        lats = list(lats.unsqueeze(1)) if lats.dim() == 4 else [lats]
    os.makedirs(a.out_dir, exist_ok=True)
    for idx, lat in enumerate(lats):
        img = dec.to_uint8(dec.decode(lat if lat.dim() == 4 else lat[None]))[0].cpu()
        path = os.path.join(a.out_dir, f"validation_{idx}.png")
        with open(path, "wb") as f:
            f.write(encode_png(img))
        print(path)
