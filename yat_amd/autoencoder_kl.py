"""AutoencoderKL decoder on the HIP path (and what the encoder, yat_amd/autoencoder_kl_encoder.py, shares with it: the
ResnetBlock2D / Attention key tables, packing and launches): the VAE decode of the PixArt-Sigma and SD3.5 validation images
(train_pixart_sigma.py:137-144, train_sd35.py:150-156), ``vae.decode(latent / vae.config.scaling_factor)`` ->
``image_processor.postprocess``, with the VAE in bf16.

    python -m yat_amd.autoencoder_kl --vae PIPE/vae models/<step>/validation_latents.pt OUT_DIR      # latents -> PNGs

What it restates [RECALL, diffusers AutoencoderKL.decode / Decoder, as the oracle restates its other modules; driven by
``vae/config.json``; any other up-block type or activation is refused]:
* ``z = bf16(latent / scaling_factor)``; ``post_quant_conv`` (1x1, bias) when ``use_post_quant_conv``;
* ``conv_in`` (3x3, latent -> C[-1]);
* ``mid_block``: resnet -> attention (``mid_block_add_attention``) -> resnet, where
  resnet = GroupNorm -> SiLU -> conv1 -> GroupNorm -> SiLU -> conv2, + the input (or its 1x1 ``conv_shortcut`` when the
  widths differ), and attention = group_norm -> to_q / to_k / to_v (bias) -> SDPA (one head of C) -> to_out.0 (bias) -> +
  the input;
* ``up_blocks`` over the reversed widths: ``layers_per_block + 1`` resnets, then ``Upsample2D`` (nearest x2 -> 3x3 conv)
  on all but the last;
* ``conv_norm_out`` (GroupNorm) -> SiLU -> ``conv_out`` (3x3 -> 3);
* every module output rounded to bf16 as the bf16 VAE rounds it; GroupNorm eps 1e-6, ``norm_num_groups`` groups.

Hot path: GroupNorm (+ SiLU) and the single-head attention are this library's KL kernels (csrc/vae_kl.hip); every 3x3 conv
runs on yat_dcae_conv3x3 (the upsampler's nearest x2 in its address math, conv2's residual in its epilogue, conv_out on the
direct small-Cout kernel), post_quant_conv / conv_shortcut / to_q|to_k|to_v (fused) / to_out.0 (+ residual) on the GEMM
family.  The conv and the GEMM want channel counts that are multiples of 8, so a 4-channel latent (PixArt-Sigma, SDXL) is
zero-padded to 8 channels at load, in post_quant_conv's weight and bias and in conv_in's weight, and in the input: the
padded channels stay exactly zero and contribute exactly zero.

The SD3.5 reference divides by ``scaling_factor`` and does NOT add ``shift_factor`` back before decoding
(train_sd35.py:155), although diffusers' own SD3 pipeline does; this decoder keeps the reference's outward contract: the
pre-scale is ``latent / scaling_factor`` for every KL VAE, ``shift_factor`` is parsed and never applied.

Directory loading, the strict key check, the buffer cache, ``decode_validation`` and the command line:
yat_amd/vae_common.py.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .vae_common import (BF16, VAEHalfHIP, check_expected, decode_validation, latents_to_png_main, load_tensors,  # noqa: F401
                         pack_conv3x3, read_config, to_uint8)

EPS = 1e-6
UP = "UpDecoderBlock2D"
ATTN_DIMS = (64, 512)            # single-head attention widths the library builds (yat_vae_attn_fwd)
# diffusers' deprecated attention names (old checkpoints) -> the current ones [RECALL: its deprecated-attention conversion]
DEPRECATED_ATTN = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


@dataclass(frozen=True)
class KLDecoderConfig:
    latent_channels: int
    block_out_channels: tuple
    layers_per_block: int
    norm_num_groups: int
    scaling_factor: float
    shift_factor: float | None
    use_post_quant_conv: bool
    mid_block_add_attention: bool
    out_channels: int = 3

    @property
    def num_blocks(self) -> int:
        return len(self.block_out_channels)

    @property
    def latent_padded(self) -> int:
        """latent channels as the conv / GEMM see them: rounded up to a multiple of 8 (zero channels)"""
        return (self.latent_channels + 7) // 8 * 8

    @property
    def upsample_factor(self) -> int:
        return 1 << (self.num_blocks - 1)


def parse_config(raw: dict) -> KLDecoderConfig:
    """``vae/config.json`` (AutoencoderKL) -> the decoder's configuration (diffusers' defaults for absent keys)."""
    chans = tuple(int(c) for c in raw.get("block_out_channels", (64,)))
    ups = tuple(raw.get("up_block_types", (UP,) * len(chans)))
    if len(ups) != len(chans):
        raise ValueError(f"up_block_types: {len(ups)} entries for {len(chans)} widths")
    bad = [t for t in ups if t != UP]
    if bad:
        raise NotImplementedError(f"up_block_types {bad[0]!r} (built: {UP!r})")
    act = raw.get("act_fn", "silu")
    if act != "silu":
        raise NotImplementedError(f"act_fn {act!r} (built: 'silu')")
    shift = raw.get("shift_factor")
    cfg = KLDecoderConfig(
        latent_channels=int(raw.get("latent_channels", 4)), block_out_channels=chans,
        layers_per_block=int(raw.get("layers_per_block", 1)), norm_num_groups=int(raw.get("norm_num_groups", 32)),
        scaling_factor=float(raw.get("scaling_factor", 0.18215)), shift_factor=None if shift is None else float(shift),
        use_post_quant_conv=bool(raw.get("use_post_quant_conv", True)),
        mid_block_add_attention=bool(raw.get("mid_block_add_attention", True)), out_channels=int(raw.get("out_channels", 3)))
    _validate(cfg)
    return cfg


def validate_widths(cfg) -> None:
    """The checks both halves share (the encoder's configuration has the same fields): GroupNorm groups, conv / GEMM
    widths, the mid-block attention width."""
    g = cfg.norm_num_groups
    for c in cfg.block_out_channels:
        if g <= 0 or c % g:
            raise NotImplementedError(f"norm_num_groups {g} does not divide the width {c}")
        if c % 8 or c > 2048:
            raise NotImplementedError(f"width {c} (built: multiples of 8 up to 2048)")
    mid = cfg.block_out_channels[-1]
    if cfg.mid_block_add_attention and mid not in ATTN_DIMS:
        raise NotImplementedError(f"mid-block width {mid}: the single-head attention is built for {ATTN_DIMS}")
    if cfg.layers_per_block <= 0:
        raise NotImplementedError(f"layers_per_block {cfg.layers_per_block}")
    if cfg.latent_channels <= 0:
        raise ValueError(f"latent_channels {cfg.latent_channels}")


def _validate(cfg: KLDecoderConfig) -> None:
    validate_widths(cfg)
    if cfg.out_channels != 3:
        raise NotImplementedError(f"out_channels {cfg.out_channels} (built: 3)")


def resnet_keys(p, cin, cout):
    """ResnetBlock2D under the prefix ``p`` -> {key: shape}."""
    k = {p + "norm1.weight": (cin,), p + "norm1.bias": (cin,), p + "conv1.weight": (cout, cin, 3, 3), p + "conv1.bias": (cout,),
         p + "norm2.weight": (cout,), p + "norm2.bias": (cout,), p + "conv2.weight": (cout, cout, 3, 3),
         p + "conv2.bias": (cout,)}
    if cin != cout:
        k.update({p + "conv_shortcut.weight": (cout, cin, 1, 1), p + "conv_shortcut.bias": (cout,)})
    return k


def attention_keys(a, c):
    """The mid-block Attention of width ``c`` under the prefix ``a`` (current names) -> {key: shape}."""
    keys = {a + "group_norm.weight": (c,), a + "group_norm.bias": (c,)}
    for t in ("to_q", "to_k", "to_v", "to_out.0"):
        keys.update({a + t + ".weight": (c, c), a + t + ".bias": (c,)})
    return keys


def _resnets(cfg: KLDecoderConfig):
    """(state-dict prefix, in width, out width) of every resnet, in decode order, and the upsamplers' (prefix, width)."""
    ch = cfg.block_out_channels
    mid = ch[-1]
    res = [("decoder.mid_block.resnets.0.", mid, mid), ("decoder.mid_block.resnets.1.", mid, mid)]
    ups = []
    rev = list(reversed(ch))
    prev = rev[0]
    for i, c in enumerate(rev):
        for j in range(cfg.layers_per_block + 1):
            res.append((f"decoder.up_blocks.{i}.resnets.{j}.", prev if j == 0 else c, c))
        if i < len(rev) - 1:
            ups.append((f"decoder.up_blocks.{i}.upsamplers.0.conv.", c))
        prev = c
    return res, ups


def expected_keys(cfg: KLDecoderConfig) -> dict:
    """Every ``decoder.*`` / ``post_quant_conv.*`` key of the diffusers state dict (current attention names) -> its shape."""
    ch, lat = cfg.block_out_channels, cfg.latent_channels
    keys = {}
    if cfg.use_post_quant_conv:
        keys.update({"post_quant_conv.weight": (lat, lat, 1, 1), "post_quant_conv.bias": (lat,)})
    keys.update({"decoder.conv_in.weight": (ch[-1], lat, 3, 3), "decoder.conv_in.bias": (ch[-1],)})
    res, ups = _resnets(cfg)
    for p, cin, cout in res:
        keys.update(resnet_keys(p, cin, cout))
    if cfg.mid_block_add_attention:
        keys.update(attention_keys("decoder.mid_block.attentions.0.", ch[-1]))
    for p, c in ups:
        keys.update({p + "weight": (c, c, 3, 3), p + "bias": (c,)})
    keys.update({"decoder.conv_norm_out.weight": (ch[0],), "decoder.conv_norm_out.bias": (ch[0],),
                 "decoder.conv_out.weight": (cfg.out_channels, ch[0], 3, 3), "decoder.conv_out.bias": (cfg.out_channels,)})
    return keys


def _ours(k: str) -> bool:
    return k.startswith("decoder.") or k.startswith("post_quant_conv.")


def convert_deprecated(sd: dict, half: str = "decoder") -> dict:
    """Old diffusers checkpoints name the mid-block attention of ``half`` ('decoder' / 'encoder') ``query`` / ``key`` /
    ``value`` / ``proj_attn``, sometimes as 1x1-conv tensors [C, C, 1, 1]: renamed to ``to_q`` / ``to_k`` / ``to_v`` /
    ``to_out.0`` with Linear shapes.  Other keys pass through unchanged."""
    out = {}
    for k, v in sd.items():
        if k.startswith(half + ".mid_block.attentions."):
            head, _, leaf = k.rpartition(".")                  # e.g. (decoder.mid_block.attentions.0.query, weight)
            base, _, name = head.rpartition(".")
            if name in DEPRECATED_ATTN:
                k = f"{base}.{DEPRECATED_ATTN[name]}.{leaf}"
                if leaf == "weight" and v.dim() == 4:
                    v = v.reshape(v.shape[0], v.shape[1])
        if k in out:
            raise KeyError(f"AutoencoderKL weight {k!r} is present under both its current and its deprecated name")
        out[k] = v
    return out


def check_state(cfg: KLDecoderConfig, sd: dict) -> None:
    """Strict load: every expected key present with its shape, and no other ``decoder.`` / ``post_quant_conv.`` key (encoder
    and quant_conv keys are ignored).  ``sd`` uses the current names (``convert_deprecated``).  Raises KeyError / ValueError
    naming the key."""
    check_expected(expected_keys(cfg), sd, _ours, "AutoencoderKL decoder", "this decoder")


def pad_latent_channels(t: torch.Tensor, n: int, dim: int) -> torch.Tensor:
    """``t`` zero-padded along ``dim`` to ``n`` entries (exact: the added channels are zeros)."""
    if t.shape[dim] == n:
        return t
    shape = list(t.shape)
    shape[dim] = n - t.shape[dim]
    return torch.cat([t, t.new_zeros(shape)], dim)


def pack_resnet(b: dict, p: str, q: str, cin: int, cout: int) -> dict:
    """ResnetBlock2D ``p`` of the bf16 state dict ``b`` -> its packed weights under the prefix ``q``."""
    out = {q + "norm1.w": b[p + "norm1.weight"], q + "norm1.b": b[p + "norm1.bias"],
           q + "conv1.w": pack_conv3x3(b[p + "conv1.weight"]), q + "conv1.b": b[p + "conv1.bias"],
           q + "norm2.w": b[p + "norm2.weight"], q + "norm2.b": b[p + "norm2.bias"],
           q + "conv2.w": pack_conv3x3(b[p + "conv2.weight"]), q + "conv2.b": b[p + "conv2.bias"]}
    if cin != cout:
        out[q + "sc.w"] = b[p + "conv_shortcut.weight"].reshape(cout, cin).contiguous()
        out[q + "sc.b"] = b[p + "conv_shortcut.bias"]
    return out


def pack_attention(b: dict, a: str) -> dict:
    """The mid-block Attention ``a`` of the bf16 state dict ``b`` -> ``attn.*``: to_q | to_k | to_v fused."""
    return {"attn.gn.w": b[a + "group_norm.weight"], "attn.gn.b": b[a + "group_norm.bias"],
            "attn.qkv.w": torch.cat([b[a + t + ".weight"] for t in ("to_q", "to_k", "to_v")], 0).contiguous(),
            "attn.qkv.b": torch.cat([b[a + t + ".bias"] for t in ("to_q", "to_k", "to_v")], 0).contiguous(),
            "attn.out.w": b[a + "to_out.0.weight"].contiguous(), "attn.out.b": b[a + "to_out.0.bias"]}


def pack_weights(cfg: KLDecoderConfig, sd: dict) -> dict:
    """Deprecated-name conversion, strict check and the one-time re-pack on the host, in bf16: 3x3 convs to [Cout, 3, 3, Cin],
    1x1 convs and Linears to [N, K], to_q | to_k | to_v fused, the latent channels padded to a multiple of 8."""
    sd = convert_deprecated({k: v for k, v in sd.items() if _ours(k)})
    check_state(cfg, sd)
    b = {k: v.to(BF16) for k, v in sd.items()}
    L, Lp = cfg.latent_channels, cfg.latent_padded
    out = {}
    if cfg.use_post_quant_conv:
        w = b["post_quant_conv.weight"].reshape(L, L)
        out["pqc.w"] = pad_latent_channels(pad_latent_channels(w, Lp, 0), Lp, 1).contiguous()
        out["pqc.b"] = pad_latent_channels(b["post_quant_conv.bias"], Lp, 0).contiguous()
    out["conv_in.w"] = pack_conv3x3(pad_latent_channels(b["decoder.conv_in.weight"], Lp, 1))
    out["conv_in.b"] = b["decoder.conv_in.bias"]
    res, ups = _resnets(cfg)
    for p, cin, cout in res:
        out.update(pack_resnet(b, p, p[len("decoder."):], cin, cout))
    if cfg.mid_block_add_attention:
        out.update(pack_attention(b, "decoder.mid_block.attentions.0."))
    for p, c in ups:
        q = p[len("decoder."):]
        out[q + "w"] = pack_conv3x3(b[p + "weight"])
        out[q + "b"] = b[p + "bias"]
    out.update({"norm_out.w": b["decoder.conv_norm_out.weight"], "norm_out.b": b["decoder.conv_norm_out.bias"],
                "conv_out.w": pack_conv3x3(b["decoder.conv_out.weight"]), "conv_out.b": b["decoder.conv_out.bias"]})
    return {k: v.contiguous() for k, v in out.items()}


def load_vae_dir(vae_dir: str):
    """(config, ``decoder.*`` + ``post_quant_conv.*`` tensors) of a diffusers AutoencoderKL directory."""
    return parse_config(read_config(vae_dir)), load_tensors(vae_dir, _ours)


class KLBlocksHIP(VAEHalfHIP):
    """What both AutoencoderKL halves run on (yat_amd/autoencoder_kl_encoder.py is the other): GroupNorm, ResnetBlock2D and
    the mid-block Attention over the packed weights ``self.w`` and the buffers ``t`` / ``u`` / ``ws`` of ``_alloc_buffers``."""

    def _gn(self, x, y, npx, c, key, silu, bf):
        from . import ops
        ops.vae_groupnorm(x, self.w[key + ".w"], self.w[key + ".b"], y, 1, npx, c, self.cfg.norm_num_groups, bf["ws"], EPS,
                          silu=silu)

    def _resnet(self, x, out, q, hh, ww, cin, cout, bf):
        """ResnetBlock2D: x [hh*ww, cin] -> out [hh*ww, cout]."""
        from . import ops
        npx = hh * ww
        x = x[:npx * cin]
        t, u = bf["t"][:npx * cin], bf["u"][:npx * cout]
        self._gn(x, t, npx, cin, q + "norm1", True, bf)
        ops.dcae_conv3x3(t, self.w[q + "conv1.w"], u, 1, hh, ww, cin, cout, bias=self.w[q + "conv1.b"])
        self._gn(u, u, npx, cout, q + "norm2", True, bf)
        res = x
        if cin != cout:                                     # conv_shortcut (1x1, bias) of the input, into t (free again)
            res = bf["t"][:npx * cout]
            ops.gemm(x.view(npx, cin), self.w[q + "sc.w"], res.view(npx, cout), M=npx, N=cout, K=cin, bias=self.w[q + "sc.b"])
        ops.dcae_conv3x3(u, self.w[q + "conv2.w"], out[:npx * cout], 1, hh, ww, cout, cout, bias=self.w[q + "conv2.b"],
                         residual=res)

    def _attention(self, x, out, npx, c, bf):
        """The mid-block Attention (1 head of c, residual connection): x [npx, c] -> out [npx, c]."""
        from . import ops
        x = x[:npx * c]
        t = bf["t"][:npx * c].view(npx, c)
        qkv = bf["u"][:npx * 3 * c].view(npx, 3 * c)
        self._gn(x, t, npx, c, "attn.gn", False, bf)
        ops.gemm(t, self.w["attn.qkv.w"], qkv, M=npx, N=3 * c, K=c, bias=self.w["attn.qkv.b"])
        ops.vae_attn_fwd(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], t, 1, npx, c, 3 * c, c)
        ops.gemm(t, self.w["attn.out.w"], out[:npx * c].view(npx, c), M=npx, N=c, K=c, bias=self.w["attn.out.b"],
                 residual=x.view(npx, c))


class AutoencoderKLDecoderHIP(KLBlocksHIP):
    """The decoder half of AutoencoderKL in bf16 on the HIP kernels.  ``decode`` runs one image at a time on the current
    stream through activation buffers sized for the largest stage (kept between calls of the same latent size)."""
    load_vae_dir = staticmethod(load_vae_dir)
    pack_weights = staticmethod(pack_weights)

    def _alloc_buffers(self, h, w):
        from . import ops
        cfg, ch = self.cfg, self.cfg.block_out_channels
        rev = list(reversed(ch))
        # the largest activation: a block's widest input or output at its resolution, or its upsampled output
        act, hh, ww = h * w * max(ch[-1], cfg.latent_padded), h, w
        for i, c in enumerate(rev):
            prev = rev[i - 1] if i else rev[0]
            act = max(act, hh * ww * max(prev, c))
            if i < len(rev) - 1:
                hh, ww = 2 * hh, 2 * ww
                act = max(act, hh * ww * c)
        ws = max(ops.vae_groupnorm_workspace_bytes(1, hh * ww, ch[0], cfg.norm_num_groups),
                 ops.vae_groupnorm_workspace_bytes(1, h * w, ch[-1], cfg.norm_num_groups))
        e = lambda k: torch.empty(max(k, 8), dtype=BF16, device=self.device)  # noqa: E731
        return {"xa": e(act), "xb": e(act), "t": e(act), "u": e(max(act, 3 * h * w * ch[-1])),
                "z": e(h * w * cfg.latent_padded), "ws": torch.empty(max(ws, 16), dtype=torch.uint8, device=self.device)}

    def _decode_one(self, z, out, h, w):
        from . import ops
        cfg, ch = self.cfg, self.cfg.block_out_channels
        bf = self._buffers(h, w)
        L = cfg.latent_padded
        cur, other = bf["xa"], bf["xb"]
        npx = h * w
        if cfg.use_post_quant_conv:
            zq = bf["t"][:npx * L].view(npx, L)
            ops.gemm(z.view(npx, L), self.w["pqc.w"], zq, M=npx, N=L, K=L, bias=self.w["pqc.b"])
            z = zq
        mid = ch[-1]
        ops.dcae_conv3x3(z, self.w["conv_in.w"], cur[:npx * mid], 1, h, w, L, mid, bias=self.w["conv_in.b"])

        def step(fn, *a):
            nonlocal cur, other
            fn(cur, other, *a)
            cur, other = other, cur

        step(self._resnet, "mid_block.resnets.0.", h, w, mid, mid, bf)
        if cfg.mid_block_add_attention:
            step(self._attention, npx, mid, bf)
        step(self._resnet, "mid_block.resnets.1.", h, w, mid, mid, bf)
        rev = list(reversed(ch))
        hh, ww, prev = h, w, rev[0]
        for i, c in enumerate(rev):
            for j in range(cfg.layers_per_block + 1):
                step(self._resnet, f"up_blocks.{i}.resnets.{j}.", hh, ww, prev if j == 0 else c, c, bf)
            prev = c
            if i < len(rev) - 1:
                hh, ww = 2 * hh, 2 * ww
                q = f"up_blocks.{i}.upsamplers.0.conv."
                ops.dcae_conv3x3(cur, self.w[q + "w"], other[:hh * ww * c], 1, hh, ww, c, c, bias=self.w[q + "b"], upsample=True)
                cur, other = other, cur
        t = bf["t"][:hh * ww * ch[0]]
        self._gn(cur, t, hh * ww, ch[0], "norm_out", True, bf)
        ops.dcae_conv3x3(t, self.w["conv_out.w"], out, 1, hh, ww, ch[0], cfg.out_channels, bias=self.w["conv_out.b"],
                         out_nchw=True)

    # ------------------------------------------------------------------------------------------------ public
    def decode(self, latents: torch.Tensor) -> torch.Tensor:
        """[B, latent_channels, h, w] -> [B, 3, 8h, 8w] bf16 (2^(blocks-1) in general), on the decoder's device.  The division
        by ``scaling_factor`` happens here, as the reference's caller does it; ``shift_factor`` is not applied (module
        docstring)."""
        cfg = self.cfg
        if latents.dim() != 4 or latents.shape[1] != cfg.latent_channels:
            raise ValueError(f"latents must be [B, {cfg.latent_channels}, h, w], got {tuple(latents.shape)}")
        B, _, h, w = latents.shape
        f = cfg.upsample_factor
        z = pre_scale(latents.to(self.device), cfg).permute(0, 2, 3, 1)
        z = pad_latent_channels(z, cfg.latent_padded, 3).contiguous()
        out = torch.empty(B, cfg.out_channels, h * f, w * f, dtype=BF16, device=self.device)
        for b in range(B):
            zb = self._buffers(h, w)["z"][:h * w * cfg.latent_padded]
            zb.copy_(z[b].reshape(-1))
            self._decode_one(zb, out[b], h, w)
        return out


def pre_scale(latents: torch.Tensor, cfg: KLDecoderConfig) -> torch.Tensor:
    """``bf16(latent / scaling_factor)``, the argument of ``vae.decode`` in both references; no ``shift_factor`` (the SD3.5
    reference's quirk, kept: train_sd35.py:155)."""
    return (latents.float() / cfg.scaling_factor).to(BF16)


def vae_class(raw: dict) -> str:
    """'AutoencoderKL' or 'AutoencoderDC' from a ``vae/config.json``: its ``_class_name``, else the keys that only one of them
    has."""
    name = raw.get("_class_name")
    if name in ("AutoencoderKL", "AutoencoderDC"):
        return name
    if name is not None:
        raise NotImplementedError(f"VAE class {name!r} (built: 'AutoencoderKL', 'AutoencoderDC')")
    if "decoder_block_out_channels" in raw or "decoder_block_types" in raw:
        return "AutoencoderDC"
    if "block_out_channels" in raw or "up_block_types" in raw:
        return "AutoencoderKL"
    raise NotImplementedError("vae/config.json names no VAE class and has neither AutoencoderKL nor AutoencoderDC keys")


def load_vae_encoder(vae_dir: str, device="cuda"):
    """The HIP encoder for the VAE in ``vae_dir``, picked by ``vae_class``."""
    if vae_class(read_config(vae_dir)) == "AutoencoderDC":
        from .dcae_encoder import AutoencoderDCEncoderHIP
        return AutoencoderDCEncoderHIP.from_pretrained(vae_dir, device=device)
    from .autoencoder_kl_encoder import AutoencoderKLEncoderHIP
    return AutoencoderKLEncoderHIP.from_pretrained(vae_dir, device=device)


def load_vae_decoder(vae_dir: str, device="cuda"):
    """The HIP decoder for the VAE in ``vae_dir``, picked by ``vae_class``."""
    if vae_class(read_config(vae_dir)) == "AutoencoderDC":
        from .dcae import AutoencoderDCDecoderHIP
        return AutoencoderDCDecoderHIP.from_pretrained(vae_dir, device=device)
    return AutoencoderKLDecoderHIP.from_pretrained(vae_dir, device=device)


def main(argv=None) -> None:
    latents_to_png_main("python -m yat_amd.autoencoder_kl", "AutoencoderKL", AutoencoderKLDecoderHIP, argv)


if __name__ == "__main__":
    main()
