"""Torch restatement of the diffusers AutoencoderDC encoder [RECALL] for the DC-AE encoder tests, written apart from
yat_amd/dcae_encoder.py (it does not import yat_amd; ResBlock / EfficientViTBlock / RMSNorm are tests/dcae_ref.py's).
NCHW, weights in the diffusers key layout (``encoder.*``), on any torch device.

    encode(cfg, sd, images, dtype)   dtype = torch.bfloat16: the reference's bf16 VAE, every module output rounded
                                     dtype = torch.float32:  the same weights in fp32 arithmetic (the ground truth)
    -> ``vae.encode(images).latent.to(bfloat16) * scaling_factor`` (train_sana.py:81-82; the fp32 run skips the bf16 cast)

``cfg`` is a plain dict: latent_channels, block_out_channels, block_types, layers_per_block, scaling_factor (per-stage
values as lists; the "Conv" down block, qkv_multiscales (5,), head dim 32 and rms_norm / silu are the only forms restated).
"""
import torch
import torch.nn.functional as F

from tests.dcae_ref import conv, evit_block, random_block, res_block, weight_drawers


def down_block(x, sd, p, c_out):
    """DCDownBlock2d(downsample=False, shortcut=True): stride-2 conv + the group mean of the unshuffled input."""
    y = F.conv2d(x, sd[p + "conv.weight"], sd[p + "conv.bias"], stride=2, padding=1)
    g = x.shape[1] * 4 // c_out
    s = F.pixel_unshuffle(x, 2).unflatten(1, (-1, g)).mean(dim=2)
    return y + s


def encode(cfg, sd, images, dtype):
    sd = {k: v.to(images.device, dtype) for k, v in sd.items() if k.startswith("encoder.")}
    ch, n = list(cfg["block_out_channels"]), len(cfg["block_out_channels"])
    x = conv(images.to(dtype), sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"])
    for i in range(n):
        nl = cfg["layers_per_block"][i]
        for j in range(nl):
            p = f"encoder.down_blocks.{i}.{j}."
            x = res_block(x, sd, p) if cfg["block_types"][i] == "ResBlock" else evit_block(x, sd, p)
        if i < n - 1:
            x = down_block(x, sd, f"encoder.down_blocks.{i}.{nl}.", ch[i + 1])
    s = x.unflatten(1, (-1, ch[-1] // cfg["latent_channels"])).mean(dim=2)
    lat = conv(x, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"]) + s
    if dtype == torch.bfloat16:
        lat = lat.to(torch.bfloat16)
    return lat * cfg["scaling_factor"]


def random_encoder_state(cfg, seed=0, in_channels=3):
    """Random encoder weights in the diffusers layout, bf16-representable (fp32 tensors), scaled so that activations stay
    O(1) through the stack."""
    ch, n, lat = list(cfg["block_out_channels"]), len(cfg["block_out_channels"]), cfg["latent_channels"]
    sd, w, vec = weight_drawers(seed)
    w("encoder.conv_in.weight", ch[0], in_channels, 3, 3, scale=2.0)
    vec("encoder.conv_in.bias", ch[0])
    for i in range(n):
        c, nl = ch[i], cfg["layers_per_block"][i]
        for j in range(nl):
            random_block(w, vec, f"encoder.down_blocks.{i}.{j}.", cfg["block_types"][i], c)
        if i < n - 1:
            # the conv output adds to a shortcut of O(1 / sqrt(g)) magnitude; 0.7 keeps the sum O(1) stage after stage
            w(f"encoder.down_blocks.{i}.{nl}.conv.weight", ch[i + 1], c, 3, 3, scale=0.7)
            vec(f"encoder.down_blocks.{i}.{nl}.conv.bias", ch[i + 1])
    w("encoder.conv_out.weight", lat, ch[-1], 3, 3)
    vec("encoder.conv_out.bias", lat)
    return sd


def diffusers_config(cfg):
    """The ``vae/config.json`` of an AutoencoderDC with this encoder AND the decoder of the same widths (list forms of the
    per-stage keys), so that one directory serves both halves."""
    from tests import dcae_ref
    raw = dcae_ref.diffusers_config(dict(cfg, layers_per_block=cfg.get("decoder_layers_per_block", cfg["layers_per_block"])))
    raw.update({"encoder_block_types": list(cfg["block_types"]),
                "encoder_block_out_channels": list(cfg["block_out_channels"]),
                "encoder_layers_per_block": list(cfg["layers_per_block"]),
                "encoder_qkv_multiscales": [[5] if t == "EfficientViTBlock" else [] for t in cfg["block_types"]],
                "downsample_block_type": "Conv"})
    return raw


SANA_F32C32_ENC = {"latent_channels": 32, "block_out_channels": [128, 256, 512, 512, 1024, 1024],
                   "block_types": ["ResBlock"] * 3 + ["EfficientViTBlock"] * 3, "layers_per_block": [2, 2, 2, 3, 3, 3],
                   "scaling_factor": 0.41407}
