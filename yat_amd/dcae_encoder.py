"""DC-AE encoder on the HIP path: the VAE encode of feature extraction (train_sana.py:78-82),
``vae.encode(images.to(bf16)).latent.to(bf16) * vae.config.scaling_factor``, with the VAE in bf16.  The twin of
yat_amd/dcae.py (the decoder); ``python -m yat_amd.extract_latents`` drives it over image files.

What it restates [RECALL, diffusers AutoencoderDC / Encoder, as the decoder does; driven by ``vae/config.json``; any other
block or downsample type is refused]:
* ``conv_in`` (3x3, 3 -> C[0]; the weight is zero-padded to 8 input channels at load and the image to 8 channels, which
  adds exact zeros to every sum);
* stages 0 .. n-1: ``layers_per_block[i]`` blocks (``ResBlock`` / ``EfficientViTBlock``, the decoder's), then, on every
  stage but the last, ``DCDownBlock2d`` in its "Conv" form: 3x3 conv with stride 2 (C_i -> C_{i+1}) plus
  ``pixel_unshuffle(x, 2).unflatten(1, (-1, 4 C_i / C_{i+1})).mean(2)``;
* ``conv_out`` (3x3, C[-1] -> latent) plus ``x.unflatten(1, (-1, C[-1] / latent)).mean(2)``; no norm, no activation;
* every module output rounded to bf16 as the bf16 VAE rounds it.  DC-AE's ``encode`` is deterministic: the latent is the
  encoder output, nothing is sampled.

Hot path: the down blocks, ``conv_out`` and the uint8 ingest are csrc/dcae_enc.hip; everything else is what the decoder
runs on (csrc/dcae.hip, the GEMM family, yat_dwconv_glu_fwd, yat_linear_attn_fwd).

Directory loading, the strict key check and the buffer cache: yat_amd/vae_common.py.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .dcae import (HEAD, RES, alloc_buffers, block_keys, evit_block, pack_block, parse_stages, refuse_quadratic_grids,
                   res_block, validate_stages)
from .vae_common import BF16, VAEHalfHIP, check_expected, load_tensors, pack_conv3x3, read_config

IN_PAD = 8            # conv_in reads 8 input channels (Cin % 8 == 0 on the MFMA conv): RGB + 5 zero channels


@dataclass(frozen=True)
class DCAEEncoderConfig:
    in_channels: int
    latent_channels: int
    block_out_channels: tuple
    block_types: tuple
    layers_per_block: tuple
    qkv_multiscales: tuple
    downsample_block_type: str
    scaling_factor: float
    attention_head_dim: int = HEAD

    @property
    def num_stages(self) -> int:
        return len(self.block_out_channels)

    @property
    def spatial_factor(self) -> int:
        return 1 << (self.num_stages - 1)


def parse_encoder_config(raw: dict) -> DCAEEncoderConfig:
    """``vae/config.json`` (AutoencoderDC) -> the encoder's configuration (``dcae.parse_stages`` for the per-stage keys)."""
    chans, types, layers, ms = parse_stages(raw, "encoder")
    if not raw.get("out_shortcut", True):
        raise NotImplementedError("out_shortcut false: the encoder without its conv_out shortcut is not built")
    cfg = DCAEEncoderConfig(
        in_channels=int(raw.get("in_channels", 3)), latent_channels=int(raw.get("latent_channels", 32)),
        block_out_channels=chans, block_types=types, layers_per_block=layers, qkv_multiscales=ms,
        downsample_block_type=raw.get("downsample_block_type", "pixel_unshuffle"),
        scaling_factor=float(raw.get("scaling_factor", 1.0)), attention_head_dim=int(raw.get("attention_head_dim", HEAD)))
    _validate(cfg)
    return cfg


def _validate(cfg: DCAEEncoderConfig) -> None:
    if cfg.downsample_block_type != "Conv":
        raise NotImplementedError(f"downsample_block_type {cfg.downsample_block_type!r}: only 'Conv' is built "
                                  "(the pixel_unshuffle form of DCDownBlock2d is not)")
    if cfg.layers_per_block[0] <= 0:
        raise NotImplementedError("encoder stage 0: 0 layers (diffusers then makes conv_in a down block, which is not built)")
    if cfg.in_channels > IN_PAD:
        raise NotImplementedError(f"{cfg.in_channels} input channels")
    validate_stages(cfg, "encoder", "down")
    if cfg.block_out_channels[-1] % cfg.latent_channels or cfg.latent_channels % 4:
        raise ValueError(f"conv_out shortcut: {cfg.block_out_channels[-1]} % {cfg.latent_channels} != 0")


def expected_keys(cfg: DCAEEncoderConfig) -> dict:
    """Every ``encoder.*`` key of the diffusers state dict -> its shape.  The down block of stage i is the last module of
    ``encoder.down_blocks.{i}`` (index ``layers_per_block[i]``)."""
    ch, n = cfg.block_out_channels, cfg.num_stages
    keys = {"encoder.conv_in.weight": (ch[0], cfg.in_channels, 3, 3), "encoder.conv_in.bias": (ch[0],)}
    for i in range(n):
        nl = cfg.layers_per_block[i]
        for j in range(nl):
            keys.update(block_keys(f"encoder.down_blocks.{i}.{j}.", cfg.block_types[i], ch[i]))
        if i < n - 1:
            keys[f"encoder.down_blocks.{i}.{nl}.conv.weight"] = (ch[i + 1], ch[i], 3, 3)
            keys[f"encoder.down_blocks.{i}.{nl}.conv.bias"] = (ch[i + 1],)
    keys.update({"encoder.conv_out.weight": (cfg.latent_channels, ch[-1], 3, 3),
                 "encoder.conv_out.bias": (cfg.latent_channels,)})
    return keys


def check_state(cfg: DCAEEncoderConfig, sd: dict) -> None:
    """Strict load: every expected ``encoder.`` key present with its shape, and no other ``encoder.`` key (decoder keys are
    ignored).  Raises KeyError / ValueError naming the key."""
    check_expected(expected_keys(cfg), sd, lambda k: k.startswith("encoder."), "DC-AE encoder",
                   f"the {cfg.block_types} encoder")


def pad_conv_in(w: torch.Tensor) -> torch.Tensor:
    """[C0, in, 3, 3] -> [C0, 8, 3, 3] with zero weights on the added input channels (exact: they multiply zeros)."""
    out = torch.zeros(w.shape[0], IN_PAD, 3, 3, dtype=w.dtype)
    out[:, :w.shape[1]] = w
    return out


def pack_weights(cfg: DCAEEncoderConfig, sd: dict) -> dict:
    """Strict check + the one-time re-pack on the host, in bf16 (the decoder's layouts; conv_in padded to 8 channels)."""
    check_state(cfg, sd)
    b = {k: v.to(BF16) for k, v in sd.items() if k.startswith("encoder.")}
    out = {"conv_in.w": pack_conv3x3(pad_conv_in(b["encoder.conv_in.weight"])), "conv_in.b": b["encoder.conv_in.bias"],
           "conv_out.w": pack_conv3x3(b["encoder.conv_out.weight"]), "conv_out.b": b["encoder.conv_out.bias"]}
    n = cfg.num_stages
    for i in range(n):
        nl = cfg.layers_per_block[i]
        for j in range(nl):
            out.update(pack_block(b, f"encoder.down_blocks.{i}.{j}.", f"{i}.{j}.", cfg.block_types[i],
                                  cfg.block_out_channels[i]))
        if i < n - 1:
            out[f"{i}.down.w"] = pack_conv3x3(b[f"encoder.down_blocks.{i}.{nl}.conv.weight"])
            out[f"{i}.down.b"] = b[f"encoder.down_blocks.{i}.{nl}.conv.bias"]
    return out


def load_vae_dir(vae_dir: str):
    """(config, ``encoder.*`` tensors) of a diffusers AutoencoderDC directory."""
    return parse_encoder_config(read_config(vae_dir)), load_tensors(vae_dir, lambda k: k.startswith("encoder."))


def shortcut_gather_index(cin: int, cout: int):
    """The down-block shortcut as an index map: output channel o averages, for u = o g .. o g + g - 1 (g = 4 cin / cout), input
    channel u // 4 at offset (dy, dx) = ((u % 4) // 2, u % 2) of its 2 x 2 block.  -> (channel, dy, dx), each [cout, g]."""
    g = 4 * cin // cout
    u = torch.arange(cout * g).reshape(cout, g)
    return u // 4, (u % 4) // 2, u % 2


class AutoencoderDCEncoderHIP(VAEHalfHIP):
    """The encoder half of AutoencoderDC in bf16 on the HIP kernels.  ``encode`` runs one image at a time on the current
    stream through activation buffers sized for the largest stage (kept between calls of the same image size).

    The reference encodes with ``vae.enable_tiling`` only at the 2048-px resolution (train_sana.py:56-57): at 2048 px and
    above its latent is stitched from tiles, so it differs from this untiled encode along the tile seams; below that both
    encode whole."""
    load_vae_dir = staticmethod(load_vae_dir)
    pack_weights = staticmethod(pack_weights)

    def _stage_sizes(self, H, W):
        return [(H >> i, W >> i) for i in range(self.cfg.num_stages)]

    def _alloc_buffers(self, H, W):
        return alloc_buffers(self._stage_sizes(H, W), self.cfg.block_out_channels, self.cfg.block_types, self.device)

    def _check_size(self, H, W):
        f = self.cfg.spatial_factor
        if H <= 0 or W <= 0 or H % f or W % f:
            raise ValueError(f"image size {H}x{W}: height and width must be multiples of {f}")
        refuse_quadratic_grids(self._stage_sizes(H, W), self.cfg)

    def _encode_one(self, x8, out, H, W):
        """x8: [H, W, 8] bf16 (channels >= in_channels zero) -> out: [H/f, W/f, latent] bf16."""
        from . import ops
        cfg, n, ch = self.cfg, self.cfg.num_stages, self.cfg.block_out_channels
        bf = self._buffers(H, W)
        cur, other = bf["xa"], bf["xb"]
        hh, ww = H, W
        x = cur[:hh * ww * ch[0]]
        ops.dcae_conv3x3(x8, self.w["conv_in.w"], x, 1, hh, ww, IN_PAD, ch[0], bias=self.w["conv_in.b"])
        for i in range(n):
            c = ch[i]
            for j in range(cfg.layers_per_block[i]):
                blk = res_block if cfg.block_types[i] == RES else evit_block
                blk(self.w, f"{i}.{j}.", x, hh, ww, c, bf)
            if i < n - 1:
                y = other[:(hh // 2) * (ww // 2) * ch[i + 1]]
                ops.dcae_conv3x3_down(x, self.w[f"{i}.down.w"], y, 1, hh, ww, c, ch[i + 1], bias=self.w[f"{i}.down.b"])
                hh, ww = hh // 2, ww // 2
                x, cur, other = y, other, cur
        ops.dcae_conv3x3_mean(x, self.w["conv_out.w"], out, 1, hh, ww, ch[-1], cfg.latent_channels, bias=self.w["conv_out.b"])

    def _encode_batch(self, x8, H, W):
        """x8: [B, H, W, 8] bf16 -> [B, latent, H/f, W/f] bf16, multiplied by ``scaling_factor``."""
        f = self.cfg.spatial_factor
        lat = torch.empty(x8.shape[0], H // f, W // f, self.cfg.latent_channels, dtype=BF16, device=self.device)
        for b in range(x8.shape[0]):
            self._encode_one(x8[b], lat[b], H, W)
        # [B, h, w, latent] -> NCHW; .to(bf16) * scaling_factor as the reference's caller does it (train_sana.py:81-82)
        return lat.permute(0, 3, 1, 2).contiguous() * self.cfg.scaling_factor

    # ------------------------------------------------------------------------------------------------ public
    def encode(self, images: torch.Tensor) -> torch.Tensor:
        """[B, in_channels, H, W] in [-1, 1] (rounded to bf16, as ``vae.encode(images.to(vae.dtype))`` rounds it) ->
        [B, latent_channels, H/f, W/f] bf16 on the encoder's device, f = 2^(stages-1) (32 for SANA's f32c32), already
        multiplied by ``scaling_factor``."""
        cfg = self.cfg
        if images.dim() != 4 or images.shape[1] != cfg.in_channels:
            raise ValueError(f"images must be [B, {cfg.in_channels}, H, W], got {tuple(images.shape)}")
        B, _, H, W = images.shape
        self._check_size(H, W)
        x8 = torch.zeros(B, H, W, IN_PAD, dtype=BF16, device=self.device)
        x8[..., :cfg.in_channels] = images.to(self.device, BF16).permute(0, 2, 3, 1)
        return self._encode_batch(x8, H, W)

    def encode_uint8(self, image: torch.Tensor) -> torch.Tensor:
        """[H, W, 3] (or [B, H, W, 3]) uint8, as PIL hands it over -> the latent of ``encode`` on torchvision's
        ``ToTensor`` -> ``Normalize(0.5, 0.5)`` -> bf16 of that image; the conversion runs on the device."""
        from . import ops
        if self.cfg.in_channels != 3:
            raise ValueError("encode_uint8 is for 3-channel VAEs")
        if image.dtype != torch.uint8 or image.dim() not in (3, 4) or image.shape[-1] != 3:
            raise ValueError(f"image must be [H, W, 3] or [B, H, W, 3] uint8, got {tuple(image.shape)} {image.dtype}")
        u = (image if image.dim() == 4 else image[None]).to(self.device).contiguous()
        _, H, W, _ = u.shape
        self._check_size(H, W)
        return self._encode_batch(ops.dcae_image_from_uint8(u), H, W)
