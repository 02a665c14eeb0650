"""Torch restatement of the diffusers AutoencoderKL decoder [RECALL] for the KL-VAE tests, written apart from
yat_amd/autoencoder_kl.py (it does not import yat_amd).  NCHW, weights in the diffusers key layout (``decoder.*``,
``post_quant_conv.*``, current attention names), on any torch device.

    decode(cfg, sd, latent, dtype)   dtype = torch.bfloat16: the reference's bf16 VAE, every module output rounded
                                     dtype = torch.float32:  the same weights in fp32 arithmetic (the ground truth)

``cfg`` is a plain dict: latent_channels, block_out_channels, layers_per_block, norm_num_groups, scaling_factor,
shift_factor, use_post_quant_conv, mid_block_add_attention (UpDecoderBlock2D / silu are the only forms restated here).
"""
import torch
import torch.nn.functional as F

from tests.dcae_ref import postprocess, weight_drawers  # noqa: F401 (postprocess: the tests reach it through this module)

EPS = 1e-6


def group_norm(x, w, b, groups):
    return F.group_norm(x, groups, w, b, eps=EPS)


def conv(x, w, b=None, pad=1):
    return F.conv2d(x, w, b, padding=pad)


def resnet(x, sd, p, groups):
    """ResnetBlock2D (temb None, output_scale_factor 1)."""
    h = F.silu(group_norm(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], groups))
    h = conv(h, sd[p + "conv1.weight"], sd[p + "conv1.bias"])
    h = F.silu(group_norm(h, sd[p + "norm2.weight"], sd[p + "norm2.bias"], groups))
    h = conv(h, sd[p + "conv2.weight"], sd[p + "conv2.bias"])
    if p + "conv_shortcut.weight" in sd:
        x = conv(x, sd[p + "conv_shortcut.weight"], sd[p + "conv_shortcut.bias"], pad=0)
    return x + h


def attention(x, sd, a, groups):
    """Attention with AttnProcessor2_0: group_norm -> to_q/k/v -> SDPA (one head of C) -> to_out.0 -> + residual."""
    B, C, H, W = x.shape
    h = group_norm(x, sd[a + "group_norm.weight"], sd[a + "group_norm.bias"], groups)
    h = h.view(B, C, H * W).transpose(1, 2)
    q = F.linear(h, sd[a + "to_q.weight"], sd[a + "to_q.bias"])
    k = F.linear(h, sd[a + "to_k.weight"], sd[a + "to_k.bias"])
    v = F.linear(h, sd[a + "to_v.weight"], sd[a + "to_v.bias"])
    o = F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0]
    o = F.linear(o, sd[a + "to_out.0.weight"], sd[a + "to_out.0.bias"])
    return o.transpose(1, 2).reshape(B, C, H, W) + x


def pre_scale(cfg, latent, dtype):
    """``latent / scaling_factor`` in the VAE's dtype -- no shift_factor (both references)."""
    return (latent.float() / cfg["scaling_factor"]).to(dtype)


def decode(cfg, sd, latent, dtype):
    sd = {k: v.to(latent.device, dtype) for k, v in sd.items()
          if k.startswith("decoder.") or k.startswith("post_quant_conv.")}
    ch, g, n = list(cfg["block_out_channels"]), cfg["norm_num_groups"], len(cfg["block_out_channels"])
    z = pre_scale(cfg, latent, dtype)
    if cfg["use_post_quant_conv"]:
        z = conv(z, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"], pad=0)
    x = conv(z, sd["decoder.conv_in.weight"], sd["decoder.conv_in.bias"])
    x = resnet(x, sd, "decoder.mid_block.resnets.0.", g)
    if cfg["mid_block_add_attention"]:
        x = attention(x, sd, "decoder.mid_block.attentions.0.", g)
    x = resnet(x, sd, "decoder.mid_block.resnets.1.", g)
    for i in range(n):
        for j in range(cfg["layers_per_block"] + 1):
            x = resnet(x, sd, f"decoder.up_blocks.{i}.resnets.{j}.", g)
        if i < n - 1:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
            p = f"decoder.up_blocks.{i}.upsamplers.0.conv."
            x = conv(x, sd[p + "weight"], sd[p + "bias"])
    x = F.silu(group_norm(x, sd["decoder.conv_norm_out.weight"], sd["decoder.conv_norm_out.bias"], g))
    return conv(x, sd["decoder.conv_out.weight"], sd["decoder.conv_out.bias"])


def random_state(cfg, seed=0, out_channels=3):
    """Random decoder weights in the diffusers layout, bf16-representable (fp32 tensors), scaled so that activations stay
    O(1) through the stack (GroupNorm re-normalises every block input)."""
    ch, n, lat = list(cfg["block_out_channels"]), len(cfg["block_out_channels"]), cfg["latent_channels"]
    sd, w, vec = weight_drawers(seed)

    def res(p, cin, cout):
        vec(p + "norm1.weight", cin, 1.0, 0.2)
        vec(p + "norm1.bias", cin)
        w(p + "conv1.weight", cout, cin, 3, 3)
        vec(p + "conv1.bias", cout)
        vec(p + "norm2.weight", cout, 1.0, 0.2)
        vec(p + "norm2.bias", cout)
        w(p + "conv2.weight", cout, cout, 3, 3, scale=0.5)
        vec(p + "conv2.bias", cout)
        if cin != cout:
            w(p + "conv_shortcut.weight", cout, cin, 1, 1)
            vec(p + "conv_shortcut.bias", cout)

    if cfg["use_post_quant_conv"]:
        w("post_quant_conv.weight", lat, lat, 1, 1)
        vec("post_quant_conv.bias", lat)
    w("decoder.conv_in.weight", ch[-1], lat, 3, 3)
    vec("decoder.conv_in.bias", ch[-1])
    res("decoder.mid_block.resnets.0.", ch[-1], ch[-1])
    if cfg["mid_block_add_attention"]:
        a, c = "decoder.mid_block.attentions.0.", ch[-1]
        vec(a + "group_norm.weight", c, 1.0, 0.2)
        vec(a + "group_norm.bias", c)
        for t in ("to_q", "to_k", "to_v"):
            w(a + t + ".weight", c, c, scale=2.0)              # peaked enough that the softmax is not uniform
            vec(a + t + ".bias", c)
        w(a + "to_out.0.weight", c, c)
        vec(a + "to_out.0.bias", c)
    res("decoder.mid_block.resnets.1.", ch[-1], ch[-1])
    rev = list(reversed(ch))
    prev = rev[0]
    for i, c in enumerate(rev):
        for j in range(cfg["layers_per_block"] + 1):
            res(f"decoder.up_blocks.{i}.resnets.{j}.", prev if j == 0 else c, c)
        if i < n - 1:
            w(f"decoder.up_blocks.{i}.upsamplers.0.conv.weight", c, c, 3, 3)
            vec(f"decoder.up_blocks.{i}.upsamplers.0.conv.bias", c)
        prev = c
    vec("decoder.conv_norm_out.weight", ch[0], 1.0, 0.2)
    vec("decoder.conv_norm_out.bias", ch[0])
    w("decoder.conv_out.weight", out_channels, ch[0], 3, 3)
    vec("decoder.conv_out.bias", out_channels)
    return sd


def diffusers_config(cfg):
    """The ``vae/config.json`` of an AutoencoderKL with this decoder."""
    n = len(cfg["block_out_channels"])
    raw = {"_class_name": "AutoencoderKL", "in_channels": 3, "out_channels": 3, "act_fn": "silu",
           "down_block_types": ["DownEncoderBlock2D"] * n, "up_block_types": ["UpDecoderBlock2D"] * n,
           "block_out_channels": list(cfg["block_out_channels"]), "layers_per_block": cfg["layers_per_block"],
           "latent_channels": cfg["latent_channels"], "norm_num_groups": cfg["norm_num_groups"],
           "scaling_factor": cfg["scaling_factor"], "shift_factor": cfg.get("shift_factor"),
           "use_quant_conv": cfg["use_post_quant_conv"], "use_post_quant_conv": cfg["use_post_quant_conv"],
           "mid_block_add_attention": cfg["mid_block_add_attention"], "force_upcast": True, "sample_size": 1024}
    return raw


SDXL_KL = {"latent_channels": 4, "block_out_channels": [128, 256, 512, 512], "layers_per_block": 2, "norm_num_groups": 32,
           "scaling_factor": 0.13025, "shift_factor": None, "use_post_quant_conv": True, "mid_block_add_attention": True}
SD35_KL = {"latent_channels": 16, "block_out_channels": [128, 256, 512, 512], "layers_per_block": 2, "norm_num_groups": 32,
           "scaling_factor": 1.5305, "shift_factor": 0.0609, "use_post_quant_conv": False, "mid_block_add_attention": True}
