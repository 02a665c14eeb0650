"""Image files -> a cached-feature shard with VAE latents: the VAE half of the reference's feature extraction
(common/features_extractor.py:76-88 over common/dataset_fetcher.py:33-41,84-86 and train_sana.py:78-82 /
train_pixart_sigma.py:61-66 / train_sd35.py:63-77) on the HIP encoder of the VAE's class (DC-AE: SANA; AutoencoderKL:
PixArt-Sigma, SD3.5).

    python -m yat_amd.extract_latents --vae PIPE/vae --resolution 1024 --out shard-000000.tar IMAGE...
    python -m yat_amd.extract_latents --vae PIPE/vae --resolution 1024 --seed 7 [--mode] [--no-shift] --out ... IMAGE...   # KL
    python -m yat_amd.extract_latents --vae PIPE/vae --resolution 1024 --device-resize --out ... IMAGE...   # HIP resize, same bytes

Per image: PIL decode to RGB -> bucket = ``find_closest_ratio(height / width)`` over the resolution's aspect table ->
``img.resize((tw, th), Image.BILINEAR)`` (what torchvision's ``Resize((th, tw))`` does to a PIL image) -> ToTensor /
Normalize(0.5, 0.5) / bf16 and the encode on the device (``AutoencoderDCEncoderHIP.encode_uint8``) -> one shard sample
``{__key__, ratio, latent, emb}``.  The embedding comes from a sidecar file ``IMAGE_STEM.emb.pt`` next to the image: the
unpadded ``[L, C]`` bf16 rows the reference stores (train_sana.py:92-94) -- for SANA, ``python -m yat_amd.encode_prompts``
writes it from ``IMAGE_STEM.txt`` on the HIP Gemma-2 encoder; the T5 / CLIP encoders of the other recipes are not built; an
``IMAGE_STEM.pooled.pt`` beside it, when there is one, becomes the sample's ``pooled`` member (SD3.5's pooled projection).

An AutoencoderKL latent is a sample of the encoder's Gaussian: ``--seed`` seeds the generator of its noise on the device (the
same seed and images give the same shard bytes), ``--mode`` stores the distribution's mode instead, ``--no-shift`` leaves
``shift_factor`` out (PixArt-Sigma's recipe; the default subtracts it when the config has one, SD3.5's recipe).
"""
from __future__ import annotations

import argparse
import os

import torch

from .common.aspect_ratios import table_for_resolution
from .common.shards import write_shard

RESOLUTIONS = (256, 512, 1024, 2048)


def find_closest_ratio(table: dict, ratio: float) -> str:
    """common/trainer.py find_closest_ratio over ``table``: the key whose float value is nearest to ``ratio`` (first wins)."""
    best, dist = 0.6, 100
    for r in table.keys():
        d = abs(float(r) - ratio)
        if dist > d:
            best, dist = r, d
    return str(best)


def bucket_for(table: dict, height: int, width: int):
    """-> (ratio key, target height, target width) of an image of ``height`` x ``width`` pixels."""
    key = find_closest_ratio(table, height / width)
    th, tw = table[key]
    return key, int(th), int(tw)


def sidecar_path(image_path: str) -> str:
    return os.path.splitext(image_path)[0] + ".emb.pt"


def load_embedding(image_path: str) -> torch.Tensor:
    path = sidecar_path(image_path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no text embedding for {image_path!r}: the sidecar {path!r} is missing (store the "
                                "unpadded [L, C] bf16 embedding there; SANA: `python -m yat_amd.encode_prompts` writes it)")
    emb = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2:
        raise ValueError(f"{path!r}: expected an [L, C] tensor")
    return emb.to(torch.bfloat16)


def load_pooled(image_path: str):
    """The optional ``IMAGE_STEM.pooled.pt`` sidecar: a [P] tensor, or None without the file."""
    path = os.path.splitext(image_path)[0] + ".pooled.pt"
    if not os.path.isfile(path):
        return None
    pooled = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(pooled, torch.Tensor) or pooled.numel() != pooled.shape[-1]:
        raise ValueError(f"{path!r}: expected a [P] tensor")
    return pooled.reshape(-1).to(torch.bfloat16)


def resized_uint8(image_path: str, table: dict, device=None):
    """-> (ratio key, [th, tw, 3] uint8 tensor) of one image file.  ``device``: resize there with the Pillow-exact HIP kernel
    (``yat_amd.image.resize_uint8``; the same bytes, left on the device) instead of with Pillow on the host."""
    import numpy as np
    from PIL import Image
    with Image.open(image_path) as im:
        img = im.convert("RGB")
    key, th, tw = bucket_for(table, img.height, img.width)
    if device is not None:
        from .image import resize_uint8
        return key, resize_uint8(torch.from_numpy(np.array(img, dtype=np.uint8)), th, tw, device=device)
    img = img.resize((tw, th), Image.BILINEAR)
    return key, torch.from_numpy(np.array(img, dtype=np.uint8))


def extract_samples(encoder, image_paths, table: dict, first_key: int = 0, resize_device=None, **encode_options):
    """Yield one shard sample per image; ``encoder`` needs ``encode_uint8([H, W, 3] uint8, **encode_options) -> [1, C, h,
    w]``."""
    for idx, path in enumerate(image_paths):
        emb = load_embedding(path)
        pooled = load_pooled(path)
        key, u8 = resized_uint8(path, table, device=resize_device)
        latent = encoder.encode_uint8(u8, **encode_options)[0]
        sample = {"__key__": f"{first_key + idx:07d}", "ratio": key, "latent": latent.to(torch.bfloat16).cpu(), "emb": emb}
        if pooled is not None:
            sample["pooled"] = pooled
        yield sample


def encode_options(vae_cls: str, seed: int, mode: bool, no_shift: bool, device) -> dict:
    """The keyword arguments of ``encode_uint8`` for a VAE class: none for the deterministic DC-AE; for AutoencoderKL the
    seeded noise generator (or ``sample=False``) and the shift switch."""
    if vae_cls == "AutoencoderDC":
        return {}
    opts = {"sample": False} if mode else {"generator": torch.Generator(device=device).manual_seed(seed)}
    if no_shift:
        opts["apply_shift"] = False
    return opts


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m yat_amd.extract_latents",
                                 description="encode image files into one cached-feature shard (latents from the HIP DC-AE "
                                             "or AutoencoderKL encoder, text embeddings from IMAGE_STEM.emb.pt sidecars)")
    ap.add_argument("--vae", required=True, help="diffusers AutoencoderDC or AutoencoderKL directory (config.json + safetensors)")
    ap.add_argument("--resolution", type=int, required=True, choices=RESOLUTIONS, help="aspect-ratio table to bucket by")
    ap.add_argument("--out", required=True, help="shard to write (.tar)")
    ap.add_argument("--first-key", type=int, default=0, help="number of the first sample key")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=0, help="AutoencoderKL: seed of the sampling noise's generator")
    ap.add_argument("--mode", action="store_true", help="AutoencoderKL: store the distribution's mode, not a sample")
    ap.add_argument("--no-shift", action="store_true", help="AutoencoderKL: do not subtract the config's shift_factor")
    ap.add_argument("--device-resize", action="store_true",
                    help="resize on the device with the Pillow-exact HIP kernel instead of with Pillow (the same shard bytes)")
    ap.add_argument("images", nargs="+")
    a = ap.parse_args(argv)
    from .autoencoder_kl import load_vae_encoder, vae_class
    from .vae_common import read_config
    enc = load_vae_encoder(a.vae, device=a.device)
    table = table_for_resolution(a.resolution)
    opts = encode_options(vae_class(read_config(a.vae)), a.seed, a.mode, a.no_shift, a.device)
    samples = list(extract_samples(enc, a.images, table, a.first_key, resize_device=a.device if a.device_resize else None, **opts))
    write_shard(a.out, samples)
    print(f"{a.out}: {len(samples)} sample(s)")


if __name__ == "__main__":
    main()
