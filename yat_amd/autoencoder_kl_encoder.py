"""AutoencoderKL encoder on the HIP path: the VAE encode of the PixArt-Sigma and SD3.5 feature extraction
(train_pixart_sigma.py:61-66, train_sd35.py:63-77), ``vae.encode(images).latent_dist.sample()`` -> ``- shift_factor`` (SD3.5
only) -> ``* scaling_factor``, with the VAE in bf16.  The twin of yat_amd/autoencoder_kl.py (the decoder), which holds the
ResnetBlock2D / Attention code both halves run on; ``python -m yat_amd.extract_latents`` drives it over image files.

What it restates [RECALL, diffusers AutoencoderKL.encode / Encoder / DiagonalGaussianDistribution, as the decoder does;
driven by ``vae/config.json``; any other down-block type or activation is refused]:
* ``conv_in`` (3x3, 3 -> C[0]; the weight is zero-padded to 8 input channels at load and the image to 8 channels, which adds
  exact zeros to every sum);
* ``down_blocks`` over the widths: ``layers_per_block`` resnets (the first one changes the width, through its 1x1
  ``conv_shortcut``), then ``Downsample2D`` on all but the last: ``F.pad(x, (0, 1, 0, 1))`` -> 3x3 conv, stride 2, no padding;
* ``mid_block``: resnet -> attention (``mid_block_add_attention``) -> resnet;
* ``conv_norm_out`` (GroupNorm) -> SiLU -> ``conv_out`` (3x3 -> 2 latent_channels); ``quant_conv`` (1x1, bias) when
  ``use_quant_conv``: the moments;
* ``DiagonalGaussianDistribution``: mean, logvar = the two halves of the moments; ``logvar.clamp(-30, 20)``; ``std = exp(0.5
  logvar)``; ``sample = mean + std * randn`` (``mode`` = mean);
* every module output and every torch op of the tail rounded to bf16 as the bf16 VAE rounds it; GroupNorm eps 1e-6.

Hot path: ``Downsample2D`` and the sampling tail are csrc/vae_kl_enc.hip; everything else is what the decoder and the DC-AE
encoder run on (GroupNorm and attention of csrc/vae_kl.hip, yat_dcae_conv3x3, the GEMM family, yat_dcae_image_from_uint8).

Directory loading, the strict key check and the buffer cache: yat_amd/vae_common.py.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .autoencoder_kl import (KLBlocksHIP, attention_keys, convert_deprecated, pack_attention, pack_resnet, resnet_keys,
                             validate_widths)
from .dcae_encoder import IN_PAD, pad_conv_in
from .vae_common import BF16, check_expected, load_tensors, pack_conv3x3, read_config

DOWN = "DownEncoderBlock2D"


@dataclass(frozen=True)
class KLEncoderConfig:
    latent_channels: int
    block_out_channels: tuple
    layers_per_block: int
    norm_num_groups: int
    scaling_factor: float
    shift_factor: float | None
    use_quant_conv: bool
    mid_block_add_attention: bool
    in_channels: int = 3

    @property
    def num_blocks(self) -> int:
        return len(self.block_out_channels)

    @property
    def spatial_factor(self) -> int:
        return 1 << (self.num_blocks - 1)

    @property
    def moment_channels(self) -> int:
        return 2 * self.latent_channels


def parse_encoder_config(raw: dict) -> KLEncoderConfig:
    """``vae/config.json`` (AutoencoderKL) -> the encoder's configuration (diffusers' defaults for absent keys)."""
    chans = tuple(int(c) for c in raw.get("block_out_channels", (64,)))
    downs = tuple(raw.get("down_block_types", (DOWN,) * len(chans)))
    if len(downs) != len(chans):
        raise ValueError(f"down_block_types: {len(downs)} entries for {len(chans)} widths")
    bad = [t for t in downs if t != DOWN]
    if bad:
        raise NotImplementedError(f"down_block_types {bad[0]!r} (built: {DOWN!r})")
    act = raw.get("act_fn", "silu")
    if act != "silu":
        raise NotImplementedError(f"act_fn {act!r} (built: 'silu')")
    shift = raw.get("shift_factor")
    cfg = KLEncoderConfig(
        latent_channels=int(raw.get("latent_channels", 4)), block_out_channels=chans,
        layers_per_block=int(raw.get("layers_per_block", 1)), norm_num_groups=int(raw.get("norm_num_groups", 32)),
        scaling_factor=float(raw.get("scaling_factor", 0.18215)), shift_factor=None if shift is None else float(shift),
        use_quant_conv=bool(raw.get("use_quant_conv", True)),
        mid_block_add_attention=bool(raw.get("mid_block_add_attention", True)), in_channels=int(raw.get("in_channels", 3)))
    validate_widths(cfg)
    if not 0 < cfg.in_channels <= IN_PAD:
        raise NotImplementedError(f"{cfg.in_channels} input channels")
    if cfg.latent_channels % 4:
        raise NotImplementedError(f"latent_channels {cfg.latent_channels} (built: multiples of 4)")
    return cfg


def _resnets(cfg: KLEncoderConfig):
    """(state-dict prefix, in width, out width) of every resnet, in encode order, and the downsamplers' (prefix, width)."""
    ch = cfg.block_out_channels
    res, downs = [], []
    prev = ch[0]
    for i, c in enumerate(ch):
        for j in range(cfg.layers_per_block):
            res.append((f"encoder.down_blocks.{i}.resnets.{j}.", prev if j == 0 else c, c))
        if i < len(ch) - 1:
            downs.append((f"encoder.down_blocks.{i}.downsamplers.0.conv.", c))
        prev = c
    res += [("encoder.mid_block.resnets.0.", ch[-1], ch[-1]), ("encoder.mid_block.resnets.1.", ch[-1], ch[-1])]
    return res, downs


def expected_keys(cfg: KLEncoderConfig) -> dict:
    """Every ``encoder.*`` / ``quant_conv.*`` key of the diffusers state dict (current attention names) -> its shape."""
    ch, m = cfg.block_out_channels, cfg.moment_channels
    keys = {"encoder.conv_in.weight": (ch[0], cfg.in_channels, 3, 3), "encoder.conv_in.bias": (ch[0],)}
    res, downs = _resnets(cfg)
    for p, cin, cout in res:
        keys.update(resnet_keys(p, cin, cout))
    for p, c in downs:
        keys.update({p + "weight": (c, c, 3, 3), p + "bias": (c,)})
    if cfg.mid_block_add_attention:
        keys.update(attention_keys("encoder.mid_block.attentions.0.", ch[-1]))
    keys.update({"encoder.conv_norm_out.weight": (ch[-1],), "encoder.conv_norm_out.bias": (ch[-1],),
                 "encoder.conv_out.weight": (m, ch[-1], 3, 3), "encoder.conv_out.bias": (m,)})
    if cfg.use_quant_conv:
        keys.update({"quant_conv.weight": (m, m, 1, 1), "quant_conv.bias": (m,)})
    return keys


def _ours(k: str) -> bool:
    return k.startswith("encoder.") or k.startswith("quant_conv.")


def check_state(cfg: KLEncoderConfig, sd: dict) -> None:
    """Strict load: every expected key present with its shape, and no other ``encoder.`` / ``quant_conv.`` key (decoder and
    post_quant_conv keys are ignored).  ``sd`` uses the current names (``convert_deprecated``).  Raises KeyError /
    ValueError naming the key."""
    check_expected(expected_keys(cfg), sd, _ours, "AutoencoderKL encoder", "this encoder")


def pack_weights(cfg: KLEncoderConfig, sd: dict) -> dict:
    """Deprecated-name conversion, strict check and the one-time re-pack on the host, in bf16 (the decoder's layouts; conv_in
    padded to 8 input channels)."""
    sd = convert_deprecated({k: v for k, v in sd.items() if _ours(k)}, "encoder")
    check_state(cfg, sd)
    b = {k: v.to(BF16) for k, v in sd.items()}
    m = cfg.moment_channels
    out = {"conv_in.w": pack_conv3x3(pad_conv_in(b["encoder.conv_in.weight"])), "conv_in.b": b["encoder.conv_in.bias"]}
    res, downs = _resnets(cfg)
    for p, cin, cout in res:
        out.update(pack_resnet(b, p, p[len("encoder."):], cin, cout))
    for p, c in downs:
        q = p[len("encoder."):]
        out[q + "w"] = pack_conv3x3(b[p + "weight"])
        out[q + "b"] = b[p + "bias"]
    if cfg.mid_block_add_attention:
        out.update(pack_attention(b, "encoder.mid_block.attentions.0."))
    out.update({"norm_out.w": b["encoder.conv_norm_out.weight"], "norm_out.b": b["encoder.conv_norm_out.bias"],
                "conv_out.w": pack_conv3x3(b["encoder.conv_out.weight"]), "conv_out.b": b["encoder.conv_out.bias"]})
    if cfg.use_quant_conv:
        out.update({"qc.w": b["quant_conv.weight"].reshape(m, m), "qc.b": b["quant_conv.bias"]})
    return {k: v.contiguous() for k, v in out.items()}


def load_vae_dir(vae_dir: str):
    """(config, ``encoder.*`` + ``quant_conv.*`` tensors) of a diffusers AutoencoderKL directory."""
    return parse_encoder_config(read_config(vae_dir)), load_tensors(vae_dir, _ours)


class AutoencoderKLEncoderHIP(KLBlocksHIP):
    """The encoder half of AutoencoderKL in bf16 on the HIP kernels.  ``encode`` runs one image at a time on the current
    stream through activation buffers sized for the largest stage (kept between calls of the same image size)."""
    load_vae_dir = staticmethod(load_vae_dir)
    pack_weights = staticmethod(pack_weights)

    def _alloc_buffers(self, H, W):
        from . import ops
        cfg, ch = self.cfg, self.cfg.block_out_channels
        act = ws = 0
        prev = ch[0]
        for i, c in enumerate(ch):                          # a block's widest input or output at its resolution
            npx = (H >> i) * (W >> i)
            act = max(act, npx * max(prev, c))
            ws = max(ws, *(ops.vae_groupnorm_workspace_bytes(1, npx, k, cfg.norm_num_groups) for k in {prev, c}))
            prev = c
        h, w = H >> (len(ch) - 1), W >> (len(ch) - 1)
        e = lambda k: torch.empty(max(k, 8), dtype=BF16, device=self.device)  # noqa: E731
        return {"xa": e(act), "xb": e(act), "t": e(act), "u": e(max(act, 3 * h * w * ch[-1])),
                "ws": torch.empty(max(ws, 16), dtype=torch.uint8, device=self.device)}

    def _check_size(self, H, W):
        f = self.cfg.spatial_factor
        if H <= 0 or W <= 0 or H % f or W % f:
            raise ValueError(f"image size {H}x{W}: height and width must be multiples of {f}")

    def _moments_one(self, x8, H, W):
        """x8: [H, W, 8] bf16 (channels >= in_channels zero) -> the moments [H/f * W/f, 2 latent] bf16, NHWC, in a buffer
        that the next call overwrites."""
        from . import ops
        cfg, ch = self.cfg, self.cfg.block_out_channels
        bf = self._buffers(H, W)
        cur, other = bf["xa"], bf["xb"]
        hh, ww = H, W
        ops.dcae_conv3x3(x8, self.w["conv_in.w"], cur[:hh * ww * ch[0]], 1, hh, ww, IN_PAD, ch[0], bias=self.w["conv_in.b"])

        def step(fn, *a):
            nonlocal cur, other
            fn(cur, other, *a)
            cur, other = other, cur

        prev = ch[0]
        for i, c in enumerate(ch):
            for j in range(cfg.layers_per_block):
                step(self._resnet, f"down_blocks.{i}.resnets.{j}.", hh, ww, prev if j == 0 else c, c, bf)
            prev = c
            if i < len(ch) - 1:
                q = f"down_blocks.{i}.downsamplers.0.conv."
                ops.vae_conv3x3_down(cur[:hh * ww * c], self.w[q + "w"], other[:(hh // 2) * (ww // 2) * c], 1, hh, ww, c, c,
                                     bias=self.w[q + "b"])
                hh, ww = hh // 2, ww // 2
                cur, other = other, cur
        mid, npx, m = ch[-1], hh * ww, cfg.moment_channels
        step(self._resnet, "mid_block.resnets.0.", hh, ww, mid, mid, bf)
        if cfg.mid_block_add_attention:
            step(self._attention, npx, mid, bf)
        step(self._resnet, "mid_block.resnets.1.", hh, ww, mid, mid, bf)
        t = bf["t"][:npx * mid]
        self._gn(cur, t, npx, mid, "norm_out", True, bf)
        mom = bf["u"][:npx * m].view(npx, m)
        ops.dcae_conv3x3(t, self.w["conv_out.w"], mom, 1, hh, ww, mid, m, bias=self.w["conv_out.b"])
        if cfg.use_quant_conv:
            mq = bf["t"][:npx * m].view(npx, m)
            ops.gemm(mom, self.w["qc.w"], mq, M=npx, N=m, K=m, bias=self.w["qc.b"])
            mom = mq
        return mom

    def _images8(self, images):
        cfg = self.cfg
        if images.dim() != 4 or images.shape[1] != cfg.in_channels:
            raise ValueError(f"images must be [B, {cfg.in_channels}, H, W], got {tuple(images.shape)}")
        B, _, H, W = images.shape
        self._check_size(H, W)
        x8 = torch.zeros(B, H, W, IN_PAD, dtype=BF16, device=self.device)
        x8[..., :cfg.in_channels] = images.to(self.device, BF16).permute(0, 2, 3, 1)
        return x8

    def _uint8_images8(self, image):
        from . import ops
        if self.cfg.in_channels != 3:
            raise ValueError("encode_uint8 is for 3-channel VAEs")
        if image.dtype != torch.uint8 or image.dim() not in (3, 4) or image.shape[-1] != 3:
            raise ValueError(f"image must be [H, W, 3] or [B, H, W, 3] uint8, got {tuple(image.shape)} {image.dtype}")
        u = (image if image.dim() == 4 else image[None]).to(self.device).contiguous()
        self._check_size(u.shape[1], u.shape[2])
        return ops.dcae_image_from_uint8(u)

    def _encode_batch(self, x8, noise, generator, sample, apply_shift):
        from . import ops
        cfg, f, L = self.cfg, self.cfg.spatial_factor, self.cfg.latent_channels
        B, H, W, _ = x8.shape
        h, w = H // f, W // f
        if apply_shift is None:
            apply_shift = cfg.shift_factor is not None
        if apply_shift and cfg.shift_factor is None:
            raise ValueError("apply_shift: this VAE's config has no shift_factor")
        shape = (B, L, h, w)
        if not sample:
            noise = None
        elif noise is None:
            # diffusers' randn_tensor: drawn on the generator's device (the layout's device without one), in the VAE's dtype
            where = generator.device if generator is not None else self.device
            noise = torch.randn(shape, generator=generator, device=where, dtype=BF16).to(self.device)
        else:
            if tuple(noise.shape) != shape:
                raise ValueError(f"noise must be {shape}, got {tuple(noise.shape)}")
            noise = noise.to(self.device, BF16).contiguous()
        out = torch.empty(shape, dtype=BF16, device=self.device)
        for b in range(B):
            mom = self._moments_one(x8[b], H, W)
            ops.vae_kl_sample(mom, None if noise is None else noise[b], out[b], 1, h * w, L, mom.shape[1],
                              cfg.scaling_factor, shift=cfg.shift_factor if apply_shift else None)
        return out

    # ------------------------------------------------------------------------------------------------ public
    def moments(self, images: torch.Tensor) -> torch.Tensor:
        """[B, in_channels, H, W] -> [B, 2 latent_channels, H/f, W/f] bf16: the argument of ``DiagonalGaussianDistribution``
        (the mean in the first half of the channels, the logvar in the second)."""
        x8 = self._images8(images)
        B, H, W, _ = x8.shape
        f, m = self.cfg.spatial_factor, self.cfg.moment_channels
        out = torch.empty(B, H // f, W // f, m, dtype=BF16, device=self.device)
        for b in range(B):
            out[b].view(-1, m).copy_(self._moments_one(x8[b], H, W))
        return out.permute(0, 3, 1, 2).contiguous()

    def encode(self, images: torch.Tensor, *, noise=None, generator=None, sample=True, apply_shift=None) -> torch.Tensor:
        """[B, in_channels, H, W] in [-1, 1] (rounded to bf16, as the bf16 VAE sees it) -> [B, latent_channels, H/f, W/f] bf16
        on the encoder's device, f = 2^(blocks-1) (8 for the SD family): ``latent_dist.sample()``, minus ``shift_factor``
        when ``apply_shift`` (default: the config has one), times ``scaling_factor``.  ``noise`` [B, latent, H/f, W/f] is the
        sample's standard-normal draw; without it, it is drawn as diffusers' ``randn_tensor`` draws it, from ``generator``
        (or the global generator of the device).  ``sample=False``: ``latent_dist.mode()`` instead."""
        return self._encode_batch(self._images8(images), noise, generator, sample, apply_shift)

    def encode_uint8(self, image: torch.Tensor, *, noise=None, generator=None, sample=True, apply_shift=None) -> torch.Tensor:
        """[H, W, 3] (or [B, H, W, 3]) uint8, as PIL hands it over -> the latent of ``encode`` on torchvision's
        ``ToTensor`` -> ``Normalize(0.5, 0.5)`` -> bf16 of that image; the conversion runs on the device."""
        return self._encode_batch(self._uint8_images8(image), noise, generator, sample, apply_shift)
