"""Image files -> a cached-feature shard with DC-AE latents: the VAE half of the reference's feature extraction
(common/features_extractor.py:76-88 over common/dataset_fetcher.py:33-41,84-86 and train_sana.py:78-82) on the HIP encoder.

    python -m yat_amd.extract_latents --vae PIPE/vae --resolution 1024 --out shard-000000.tar IMAGE...

Per image: PIL decode to RGB -> bucket = ``find_closest_ratio(height / width)`` over the resolution's aspect table ->
``img.resize((tw, th), Image.BILINEAR)`` (what torchvision's ``Resize((th, tw))`` does to a PIL image) -> ToTensor /
Normalize(0.5, 0.5) / bf16 and the encode on the device (``AutoencoderDCEncoderHIP.encode_uint8``) -> one shard sample
``{__key__, ratio, latent, emb}``.  The text encoder is not built, so the embedding comes from a sidecar file
``IMAGE_STEM.emb.pt`` next to the image: the unpadded ``[L, C]`` bf16 rows the reference stores (train_sana.py:92-94).
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
        raise FileNotFoundError(f"no text embedding for {image_path!r}: the sidecar {path!r} is missing (the text encoder is "
                                "not built; store the unpadded [L, C] bf16 embedding there)")
    emb = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2:
        raise ValueError(f"{path!r}: expected an [L, C] tensor")
    return emb.to(torch.bfloat16)


def resized_uint8(image_path: str, table: dict):
    """-> (ratio key, [th, tw, 3] uint8 tensor) of one image file."""
    import numpy as np
    from PIL import Image
    with Image.open(image_path) as im:
        img = im.convert("RGB")
    key, th, tw = bucket_for(table, img.height, img.width)
    img = img.resize((tw, th), Image.BILINEAR)
    return key, torch.from_numpy(np.array(img, dtype=np.uint8))


def extract_samples(encoder, image_paths, table: dict, first_key: int = 0):
    """Yield one shard sample per image; ``encoder`` needs ``encode_uint8([H, W, 3] uint8) -> [1, C, h, w]``."""
    for idx, path in enumerate(image_paths):
        emb = load_embedding(path)
        key, u8 = resized_uint8(path, table)
        latent = encoder.encode_uint8(u8)[0]
        yield {"__key__": f"{first_key + idx:07d}", "ratio": key, "latent": latent.to(torch.bfloat16).cpu(), "emb": emb}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m yat_amd.extract_latents",
                                 description="encode image files into one cached-feature shard (latents from the HIP DC-AE "
                                             "encoder, text embeddings from IMAGE_STEM.emb.pt sidecars)")
    ap.add_argument("--vae", required=True, help="diffusers AutoencoderDC directory (config.json + safetensors)")
    ap.add_argument("--resolution", type=int, required=True, choices=RESOLUTIONS, help="aspect-ratio table to bucket by")
    ap.add_argument("--out", required=True, help="shard to write (.tar)")
    ap.add_argument("--first-key", type=int, default=0, help="number of the first sample key")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("images", nargs="+")
    a = ap.parse_args(argv)
    from .dcae_encoder import AutoencoderDCEncoderHIP
    enc = AutoencoderDCEncoderHIP.from_pretrained(a.vae, device=a.device)
    table = table_for_resolution(a.resolution)
    samples = list(extract_samples(enc, a.images, table, a.first_key))
    write_shard(a.out, samples)
    print(f"{a.out}: {len(samples)} sample(s)")


if __name__ == "__main__":
    main()
