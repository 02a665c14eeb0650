"""DC-AE decoder on the HIP path: the VAE decode of SanaModel.validate (train_sana.py:153-157),
``vae.decode(latent / vae.config.scaling_factor)`` -> ``image_processor.postprocess``, with the VAE in bf16 (:60).

    python -m yat_amd.dcae --vae PIPE/vae models/<step>/validation_latents.pt OUT_DIR      # latents -> PNGs

What it restates [RECALL, diffusers AutoencoderDC / Decoder, as the oracle restates its other modules; driven by
``vae/config.json``; any other block, norm or upsample type is refused]:
* ``z = bf16(latent / scaling_factor)``; ``conv_in`` (3x3, latent -> C[-1]) + ``repeat_interleave(z, C[-1] / latent)``;
* stages n-1 .. 0: every stage but the last starts with ``DCUpBlock2d`` (interpolate mode: nearest x2 -> 3x3 conv, plus
  ``pixel_shuffle(repeat_interleave(x, 4 C_i / C_{i+1}), 2)``), then ``layers_per_block[i]`` blocks:
  ``ResBlock``: conv1 (3x3, bias) -> SiLU -> conv2 (3x3) -> RMSNorm(bias) -> + x;
  ``EfficientViTBlock``: SanaMultiscaleLinearAttention (to_q | to_k | to_v, a depthwise 5x5 + grouped 1x1 aggregate of
  the qkv, ReLU linear attention over heads of 32 in fp32, to_out, RMSNorm, + x), then GLUMBConv (conv_inverted + SiLU,
  depthwise 3x3, h * SiLU(gate), conv_point, RMSNorm, + x);
* ``norm_out`` (RMSNorm, bias) -> ReLU -> ``conv_out`` (3x3, C0 -> 3);
* every module output rounded to bf16 as the bf16 VAE rounds it.

Hot path: 3x3 convs, the multiscale aggregate, the biased RMSNorm and the postprocess are this library's DC-AE kernels
(csrc/dcae.hip); the Linears / 1x1 convs run on the GEMM family, the GLUMBConv middle on yat_dwconv_glu_fwd and the linear
attention on yat_linear_attn_fwd.  The latter wants q, k, v each head-major in separate column ranges; diffusers' qkv
reshape takes head g's q, k, v from 32-channel blocks 3g, 3g+1, 3g+2 of ``cat(to_q, to_k, to_v)``, so the loader moves
block 3g+j to position j*H + g in the fused qkv weight and in both aggregate convs (a block permutation commutes with
the per-channel 5x5 and the per-block 1x1).  One attention call over the base qkv and one over the aggregate then write
to_out's input columns [0, C) and [C, 2C) in diffusers' head order.

Directory loading, the strict key check, the buffer cache and the command line: yat_amd/vae_common.py.  The per-stage
config parsing and checks and the blocks below also serve the encoder (yat_amd/dcae_encoder.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .vae_common import (BF16, VAEHalfHIP, check_expected, find_vae_dir, latents_to_png_main, load_tensors,  # noqa: F401
                         pack_conv3x3, read_config, to_uint8)

RES, EVIT = "ResBlock", "EfficientViTBlock"
EPS = 1e-5
HEAD = 32


@dataclass(frozen=True)
class DCAEDecoderConfig:
    latent_channels: int
    block_out_channels: tuple
    block_types: tuple
    layers_per_block: tuple
    qkv_multiscales: tuple
    norm_types: tuple
    act_fns: tuple
    upsample_block_type: str
    scaling_factor: float
    attention_head_dim: int = HEAD
    out_channels: int = 3

    @property
    def num_stages(self) -> int:
        return len(self.block_out_channels)


def per_stage(v, n, name):
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise ValueError(f"{name}: {len(v)} entries for {n} decoder stages")
        return tuple(v)
    return (v,) * n


def parse_stages(raw: dict, side: str):
    """The per-stage keys of one half (``side``: 'decoder' / 'encoder') of an AutoencoderDC ``config.json`` -> (widths, block
    types, layers, qkv multiscales), one entry per stage.  A key may be a scalar (every stage) or a list (one entry per
    stage); ``{side}_qkv_multiscales`` a list of kernel sizes (every stage) or a list of lists."""
    chans = tuple(int(c) for c in raw[f"{side}_block_out_channels"])
    n = len(chans)
    types = per_stage(raw.get(f"{side}_block_types", RES), n, f"{side}_block_types")
    layers = tuple(int(v) for v in per_stage(raw.get(f"{side}_layers_per_block", 2), n, f"{side}_layers_per_block"))
    ms = raw.get(f"{side}_qkv_multiscales", ())
    if isinstance(ms, (list, tuple)) and ms and all(isinstance(m, (list, tuple)) for m in ms):
        ms = tuple(tuple(int(k) for k in m) for m in per_stage(list(ms), n, f"{side}_qkv_multiscales"))
    elif isinstance(ms, (list, tuple)):
        ms = (tuple(int(k) for k in ms),) * n
    else:
        ms = ((int(ms),),) * n
    return chans, types, layers, ms


def validate_stages(cfg, side: str, shortcut: str, extra=None) -> None:
    """The per-stage refusals both halves make; ``shortcut`` names the side's resampling block ('up' / 'down') and
    ``extra(i, block_type)`` makes the side's own per-stage checks, after the block-type check."""
    ch = cfg.block_out_channels
    for i, (c, t, nl, ms) in enumerate(zip(ch, cfg.block_types, cfg.layers_per_block, cfg.qkv_multiscales)):
        if t not in (RES, EVIT):
            raise NotImplementedError(f"{side} stage {i}: block type {t!r} (built: {RES}, {EVIT})")
        if extra is not None:
            extra(i, t)
        if t == EVIT and (tuple(ms) != (5,) or cfg.attention_head_dim != HEAD):
            raise NotImplementedError(f"{side} stage {i}: qkv_multiscales {ms} / head dim {cfg.attention_head_dim} "
                                      f"(built: (5,) / {HEAD})")
        if nl <= 0:
            raise NotImplementedError(f"{side} stage {i}: {nl} layers (a stage without blocks is not built)")
        if c % 8 or (t == EVIT and c % HEAD):
            raise ValueError(f"{side} stage {i}: {c} channels")
        if i + 1 < len(ch) and (4 * c) % ch[i + 1]:
            raise ValueError(f"{side} stage {i}: the {shortcut}-block shortcut needs 4*{c} % {ch[i + 1]} == 0")


def refuse_quadratic_grids(sizes, cfg) -> None:
    """``sizes``: the (h, w) of every stage.  diffusers' multiscale attention is linear only above head-dim pixels."""
    for (hh, ww), t in zip(sizes, cfg.block_types):
        if t == EVIT and hh * ww <= cfg.attention_head_dim:
            raise ValueError(f"a {hh}x{ww} grid switches diffusers' multiscale attention to its quadratic form "
                             "(h*w <= 32), which is not built")


def parse_config(raw: dict) -> DCAEDecoderConfig:
    """``vae/config.json`` (AutoencoderDC) -> the decoder's configuration (``parse_stages`` for the per-stage keys)."""
    chans, types, layers, ms = parse_stages(raw, "decoder")
    n = len(chans)
    cfg = DCAEDecoderConfig(
        latent_channels=int(raw.get("latent_channels", 32)), block_out_channels=chans, block_types=types,
        layers_per_block=layers, qkv_multiscales=ms,
        norm_types=per_stage(raw.get("decoder_norm_types", "rms_norm"), n, "decoder_norm_types"),
        act_fns=per_stage(raw.get("decoder_act_fns", "silu"), n, "decoder_act_fns"),
        upsample_block_type=raw.get("upsample_block_type", "pixel_shuffle"),
        scaling_factor=float(raw.get("scaling_factor", 1.0)), attention_head_dim=int(raw.get("attention_head_dim", HEAD)),
        out_channels=int(raw.get("in_channels", 3)))
    _validate(cfg)
    return cfg


def _validate(cfg: DCAEDecoderConfig) -> None:
    if cfg.upsample_block_type != "interpolate":
        raise NotImplementedError(f"upsample_block_type {cfg.upsample_block_type!r}: only 'interpolate' is built")

    def norm_and_act(i, t):
        if cfg.norm_types[i] != "rms_norm":
            raise NotImplementedError(f"decoder stage {i}: norm type {cfg.norm_types[i]!r} (built: 'rms_norm')")
        if t == RES and cfg.act_fns[i] != "silu":
            raise NotImplementedError(f"decoder stage {i}: activation {cfg.act_fns[i]!r} (built: 'silu')")
    validate_stages(cfg, "decoder", "up", norm_and_act)
    if cfg.block_out_channels[-1] % cfg.latent_channels or cfg.latent_channels % 8:
        raise ValueError(f"conv_in shortcut: {cfg.block_out_channels[-1]} % {cfg.latent_channels} != 0")
    if cfg.out_channels > 4:
        raise NotImplementedError(f"{cfg.out_channels} output channels")


def block_keys(p: str, block_type: str, c: int) -> dict:
    """Keys -> shapes of one ResBlock / EfficientViTBlock of width ``c`` under the diffusers prefix ``p``."""
    if block_type == RES:
        return {p + "conv1.weight": (c, c, 3, 3), p + "conv1.bias": (c,), p + "conv2.weight": (c, c, 3, 3),
                p + "norm.weight": (c,), p + "norm.bias": (c,)}
    a, g = p + "attn.", p + "conv_out."
    return {a + "to_q.weight": (c, c), a + "to_k.weight": (c, c), a + "to_v.weight": (c, c),
            a + "to_qkv_multiscale.0.proj_in.weight": (3 * c, 1, 5, 5),
            a + "to_qkv_multiscale.0.proj_out.weight": (3 * c, HEAD, 1, 1),
            a + "to_out.weight": (c, 2 * c), a + "norm_out.weight": (c,), a + "norm_out.bias": (c,),
            g + "conv_inverted.weight": (8 * c, c, 1, 1), g + "conv_inverted.bias": (8 * c,),
            g + "conv_depth.weight": (8 * c, 1, 3, 3), g + "conv_depth.bias": (8 * c,),
            g + "conv_point.weight": (c, 4 * c, 1, 1), g + "norm.weight": (c,), g + "norm.bias": (c,)}


def expected_keys(cfg: DCAEDecoderConfig) -> dict:
    """Every ``decoder.*`` key of the diffusers state dict -> its shape."""
    ch, lat, n = cfg.block_out_channels, cfg.latent_channels, cfg.num_stages
    keys = {"decoder.conv_in.weight": (ch[-1], lat, 3, 3), "decoder.conv_in.bias": (ch[-1],)}
    for i in range(n):
        c, j0 = ch[i], 0
        if i < n - 1:
            keys[f"decoder.up_blocks.{i}.0.conv.weight"] = (c, ch[i + 1], 3, 3)
            keys[f"decoder.up_blocks.{i}.0.conv.bias"] = (c,)
            j0 = 1
        for j in range(j0, j0 + cfg.layers_per_block[i]):
            keys.update(block_keys(f"decoder.up_blocks.{i}.{j}.", cfg.block_types[i], c))
    keys.update({"decoder.norm_out.weight": (ch[0],), "decoder.norm_out.bias": (ch[0],),
                 "decoder.conv_out.weight": (cfg.out_channels, ch[0], 3, 3), "decoder.conv_out.bias": (cfg.out_channels,)})
    return keys


def check_state(cfg: DCAEDecoderConfig, sd: dict) -> None:
    """Strict load: every expected ``decoder.`` key present with its shape, and no other ``decoder.`` key (encoder keys are
    ignored).  Raises KeyError / ValueError naming the key."""
    check_expected(expected_keys(cfg), sd, lambda k: k.startswith("decoder."), "DC-AE decoder",
                   f"the {cfg.block_types} decoder")


def qkv_block_perm(heads: int) -> torch.Tensor:
    """Destination position p = j*heads + g <- source block 3g + j (j = q, k, v): diffusers' per-head [q|k|v] blocks of
    cat(to_q, to_k, to_v) regrouped into q | k | v, each head-major."""
    return torch.tensor([3 * (p % heads) + p // heads for p in range(3 * heads)], dtype=torch.long)


def permute_blocks(t: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """Rows of ``t`` ([3C, ...]) regrouped in blocks of 32 by ``perm``."""
    nb = perm.numel()
    return t.reshape(nb, HEAD, *t.shape[1:])[perm].reshape(t.shape)


def pack_block(b: dict, p: str, q: str, block_type: str, c: int) -> dict:
    """The re-packed bf16 weights of one block: diffusers prefix ``p`` in ``b`` -> short names under ``q``."""
    if block_type == RES:
        return {q + "conv1.w": pack_conv3x3(b[p + "conv1.weight"]), q + "conv1.b": b[p + "conv1.bias"],
                q + "conv2.w": pack_conv3x3(b[p + "conv2.weight"]),
                q + "norm.w": b[p + "norm.weight"], q + "norm.b": b[p + "norm.bias"]}
    a, g = p + "attn.", p + "conv_out."
    perm = qkv_block_perm(c // HEAD)
    wcat = torch.cat([b[a + "to_q.weight"], b[a + "to_k.weight"], b[a + "to_v.weight"]], 0)
    return {
        q + "qkv.w": permute_blocks(wcat, perm).contiguous(),
        q + "ms_dw.w": permute_blocks(b[a + "to_qkv_multiscale.0.proj_in.weight"].reshape(3 * c, 25), perm).contiguous(),
        q + "ms_pw.w": permute_blocks(b[a + "to_qkv_multiscale.0.proj_out.weight"].reshape(3 * c, HEAD), perm).contiguous(),
        q + "to_out.w": b[a + "to_out.weight"].contiguous(),
        q + "attn_norm.w": b[a + "norm_out.weight"], q + "attn_norm.b": b[a + "norm_out.bias"],
        q + "inv.w": b[g + "conv_inverted.weight"].reshape(8 * c, c).contiguous(), q + "inv.b": b[g + "conv_inverted.bias"],
        q + "dw.w": b[g + "conv_depth.weight"].reshape(8 * c, 9).contiguous(), q + "dw.b": b[g + "conv_depth.bias"],
        q + "pt.w": b[g + "conv_point.weight"].reshape(c, 4 * c).contiguous(),
        q + "glu_norm.w": b[g + "norm.weight"], q + "glu_norm.b": b[g + "norm.bias"]}


def pack_weights(cfg: DCAEDecoderConfig, sd: dict) -> dict:
    """Strict check + the one-time re-pack (3x3 convs to [Cout, 3, 3, Cin], 1x1 convs to [N, K], fused and block-permuted
    qkv weights) on the host, in bf16.  Keys of the result: the diffusers prefix of each block + a short name."""
    check_state(cfg, sd)
    b = {k: v.to(BF16) for k, v in sd.items() if k.startswith("decoder.")}
    out = {"conv_in.w": pack_conv3x3(b["decoder.conv_in.weight"]), "conv_in.b": b["decoder.conv_in.bias"],
           "norm_out.w": b["decoder.norm_out.weight"], "norm_out.b": b["decoder.norm_out.bias"],
           "conv_out.w": pack_conv3x3(b["decoder.conv_out.weight"]), "conv_out.b": b["decoder.conv_out.bias"]}
    n = cfg.num_stages
    for i in range(n):
        c, j0 = cfg.block_out_channels[i], 0
        if i < n - 1:
            out[f"{i}.up.w"] = pack_conv3x3(b[f"decoder.up_blocks.{i}.0.conv.weight"])
            out[f"{i}.up.b"] = b[f"decoder.up_blocks.{i}.0.conv.bias"]
            j0 = 1
        for j in range(j0, j0 + cfg.layers_per_block[i]):
            out.update(pack_block(b, f"decoder.up_blocks.{i}.{j}.", f"{i}.{j}.", cfg.block_types[i], c))
    return out


def load_vae_dir(vae_dir: str):
    """(config, ``decoder.*`` tensors) of a diffusers AutoencoderDC directory."""
    return parse_config(read_config(vae_dir)), load_tensors(vae_dir, lambda k: k.startswith("decoder."))


def alloc_buffers(sizes, channels, block_types, device) -> dict:
    """Activation and scratch buffers of one image for stages of ``sizes`` [(h, w)] x ``channels``: two ping-pong
    activations, the blocks' temporaries (t1, t2; s, g, ws for the EfficientViT stages)."""
    from . import ops
    act = max(hh * ww * c for (hh, ww), c in zip(sizes, channels))
    evit = [(hh * ww, c) for (hh, ww), c, t in zip(sizes, channels, block_types) if t == EVIT]
    big = max([npx * 8 * c for npx, c in evit], default=0)
    mid = max([npx * 4 * c for npx, c in evit], default=0)
    ws = max([ops.linear_attn_workspace_bytes(1, npx, c // HEAD) for npx, c in evit], default=0)
    e = lambda k: torch.empty(max(k, 1), dtype=BF16, device=device)  # noqa: E731
    return {"xa": e(act), "xb": e(act), "t1": e(act), "t2": e(act), "s": e(big), "g": e(mid),
            "ws": torch.empty(max(ws, 16), dtype=torch.uint8, device=device)}


# ---------------------------------------------------------------------------- blocks (shared with yat_amd/dcae_encoder.py)
def res_block(w, q, x, hh, ww, c, bf):
    """ResBlock ``q`` in place on x ([hh * ww * c] NHWC) through the scratch buffers ``bf``; ``w``: the packed weights."""
    from . import ops
    t1, t2 = bf["t1"][:hh * ww * c], bf["t2"][:hh * ww * c]
    ops.dcae_conv3x3(x, w[q + "conv1.w"], t1, 1, hh, ww, c, c, bias=w[q + "conv1.b"], silu=True)
    ops.dcae_conv3x3(t1, w[q + "conv2.w"], t2, 1, hh, ww, c, c)
    x2 = x.view(hh * ww, c)
    ops.dcae_rmsnorm_bias(t2.view(hh * ww, c), w[q + "norm.w"], w[q + "norm.b"], x2, EPS, residual=x2)


def evit_block(w, q, x, hh, ww, c, bf):
    """EfficientViTBlock ``q`` in place on x."""
    from . import ops
    npx, heads = hh * ww, c // HEAD
    x2 = x.view(npx, c)
    s, g, t = bf["s"], bf["g"], bf["t1"][:npx * c].view(npx, c)
    qkv = s[:npx * 3 * c].view(npx, 3 * c)
    agg = s[npx * 3 * c:npx * 6 * c].view(npx, 3 * c)
    o = g[:npx * 2 * c].view(npx, 2 * c)
    ops.gemm(x2, w[q + "qkv.w"], qkv, M=npx, N=3 * c, K=c)                                  # to_q | to_k | to_v
    ops.dcae_msla_aggregate(qkv, w[q + "ms_dw.w"], w[q + "ms_pw.w"], agg, 1, hh, ww, 3 * c)
    ops.linear_attn_fwd(qkv, 1, npx, heads, c, 2 * c, o[:, :c], bf["ws"])                        # base heads
    ops.linear_attn_fwd(agg, 1, npx, heads, c, 2 * c, o[:, c:], bf["ws"])                        # aggregated heads
    ops.gemm(o, w[q + "to_out.w"], t, M=npx, N=c, K=2 * c)
    ops.dcae_rmsnorm_bias(t, w[q + "attn_norm.w"], w[q + "attn_norm.b"], x2, EPS, residual=x2)
    sil = s[:npx * 8 * c].view(npx, 8 * c)
    ops.gemm(x2, w[q + "inv.w"], sil, M=npx, N=8 * c, K=c, bias=w[q + "inv.b"], activation="silu")
    glu = g[:npx * 4 * c].view(npx, 4 * c)
    ops.dwconv_glu_fwd(sil, 1, hh, ww, 4 * c, w[q + "dw.w"], w[q + "dw.b"], glu)
    ops.gemm(glu, w[q + "pt.w"], t, M=npx, N=c, K=4 * c)
    ops.dcae_rmsnorm_bias(t, w[q + "glu_norm.w"], w[q + "glu_norm.b"], x2, EPS, residual=x2)


class AutoencoderDCDecoderHIP(VAEHalfHIP):
    """The decoder half of AutoencoderDC in bf16 on the HIP kernels.  ``decode`` runs one image at a time on the current
    stream through activation buffers sized for the largest stage (kept between calls of the same latent size).

    The reference decodes with ``vae.enable_tiling(2048, 2048)`` (train_sana.py:57): at 2048 px and above its output is
    stitched from tiles, so it differs from this untiled decode along the tile seams; below that both decode whole."""
    load_vae_dir = staticmethod(load_vae_dir)
    pack_weights = staticmethod(pack_weights)

    def _stage_sizes(self, h, w):
        n = self.cfg.num_stages
        return [(h << (n - 1 - i), w << (n - 1 - i)) for i in range(n)]

    def _alloc_buffers(self, h, w):
        return alloc_buffers(self._stage_sizes(h, w), self.cfg.block_out_channels, self.cfg.block_types, self.device)

    def _decode_one(self, z, out, h, w):
        from . import ops
        cfg, n, ch = self.cfg, self.cfg.num_stages, self.cfg.block_out_channels
        bf = self._buffers(h, w)
        cur, other = bf["xa"], bf["xb"]
        x = cur[:h * w * ch[-1]]
        ops.dcae_conv3x3(z, self.w["conv_in.w"], x, 1, h, w, cfg.latent_channels, ch[-1], bias=self.w["conv_in.b"],
                         shortcut_mode=1, shortcut=z, shortcut_channels=cfg.latent_channels)
        hh, ww = h, w
        for i in reversed(range(n)):
            c, j0 = ch[i], 0
            if i < n - 1:
                hh, ww = 2 * hh, 2 * ww
                y = other[:hh * ww * c]
                ops.dcae_conv3x3(x, self.w[f"{i}.up.w"], y, 1, hh, ww, ch[i + 1], c, bias=self.w[f"{i}.up.b"], upsample=True,
                                 shortcut_mode=2, shortcut=x, shortcut_channels=ch[i + 1])
                x, cur, other = y, other, cur
                j0 = 1
            for j in range(j0, j0 + cfg.layers_per_block[i]):
                blk = res_block if cfg.block_types[i] == RES else evit_block
                blk(self.w, f"{i}.{j}.", x, hh, ww, c, bf)
        t = bf["t1"][:hh * ww * ch[0]]
        ops.dcae_rmsnorm_bias(x.view(hh * ww, ch[0]), self.w["norm_out.w"], self.w["norm_out.b"], t.view(hh * ww, ch[0]),
                              EPS, relu=True)
        ops.dcae_conv3x3(t, self.w["conv_out.w"], out, 1, hh, ww, ch[0], cfg.out_channels, bias=self.w["conv_out.b"],
                         out_nchw=True)

    # ------------------------------------------------------------------------------------------------ public
    def decode(self, latents: torch.Tensor) -> torch.Tensor:
        """[B, latent_channels, h, w] -> [B, 3, 32h, 32w] bf16 (for SANA's f32c32; 2^(stages-1) in general), on the
        decoder's device.  The division by ``scaling_factor`` happens here, as the reference's caller does it."""
        cfg = self.cfg
        if latents.dim() != 4 or latents.shape[1] != cfg.latent_channels:
            raise ValueError(f"latents must be [B, {cfg.latent_channels}, h, w], got {tuple(latents.shape)}")
        B, _, h, w = latents.shape
        refuse_quadratic_grids(self._stage_sizes(h, w), cfg)
        f = 1 << (cfg.num_stages - 1)
        z = (latents.to(self.device).float() / cfg.scaling_factor).to(BF16).permute(0, 2, 3, 1).contiguous()
        out = torch.empty(B, cfg.out_channels, h * f, w * f, dtype=BF16, device=self.device)
        for b in range(B):
            self._decode_one(z[b], out[b], h, w)
        return out


def main(argv=None) -> None:
    latents_to_png_main("python -m yat_amd.dcae", "AutoencoderDC", AutoencoderDCDecoderHIP, argv)


if __name__ == "__main__":
    main()
