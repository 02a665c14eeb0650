"""Torch restatement of the diffusers AutoencoderKL encoder [RECALL] for the KL-encoder tests, written apart from
yat_amd/autoencoder_kl_encoder.py (it does not import yat_amd; ResnetBlock2D / Attention / GroupNorm are
tests/autoencoder_kl_ref.py's).  NCHW, weights in the diffusers key layout (``encoder.*``, ``quant_conv.*``, current
attention names), on any torch device.

    moments(cfg, sd, images, dtype)   dtype = torch.bfloat16: the reference's bf16 VAE, every module output rounded
                                      dtype = torch.float32:  the same weights in fp32 arithmetic (the ground truth)
    sample(mom, noise, scaling_factor, shift_factor)   DiagonalGaussianDistribution(mom).sample() with the given draw (None:
                                      .mode()), then ``- shift_factor`` (None: no shift) and ``* scaling_factor``, in mom's dtype
    encode(cfg, sd, images, dtype, noise, apply_shift)  the two chained, as the trainers' extract_latents chain them

``cfg`` is the plain dict of tests/autoencoder_kl_ref.py (``use_post_quant_conv`` also stands for ``use_quant_conv``, as in
its ``diffusers_config``; DownEncoderBlock2D / silu are the only forms restated here).
"""
import torch
import torch.nn.functional as F

from tests.autoencoder_kl_ref import SD35_KL, SDXL_KL, attention, conv, diffusers_config, group_norm, resnet  # noqa: F401
from tests.dcae_ref import weight_drawers


def downsample(x, w, b):
    """Downsample2D(use_conv=True, padding=0): one zero row below and one zero column to the right, then stride 2."""
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


def moments(cfg, sd, images, dtype):
    sd = {k: v.to(images.device, dtype) for k, v in sd.items() if k.startswith("encoder.") or k.startswith("quant_conv.")}
    g, n = cfg["norm_num_groups"], len(cfg["block_out_channels"])
    x = conv(images.to(dtype), sd["encoder.conv_in.weight"], sd["encoder.conv_in.bias"])
    for i in range(n):
        for j in range(cfg["layers_per_block"]):
            x = resnet(x, sd, f"encoder.down_blocks.{i}.resnets.{j}.", g)
        if i < n - 1:
            p = f"encoder.down_blocks.{i}.downsamplers.0.conv."
            x = downsample(x, sd[p + "weight"], sd[p + "bias"])
    x = resnet(x, sd, "encoder.mid_block.resnets.0.", g)
    if cfg["mid_block_add_attention"]:
        x = attention(x, sd, "encoder.mid_block.attentions.0.", g)
    x = resnet(x, sd, "encoder.mid_block.resnets.1.", g)
    x = F.silu(group_norm(x, sd["encoder.conv_norm_out.weight"], sd["encoder.conv_norm_out.bias"], g))
    x = conv(x, sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"])
    if cfg["use_post_quant_conv"]:
        x = conv(x, sd["quant_conv.weight"], sd["quant_conv.bias"], pad=0)
    return x


def _with_float(x, op, value):
    """``x op python_float`` as torch's device kernels compute it for a bf16 tensor: fp32 arithmetic with the scalar as
    (float)value, one rounding.  Written out because torch's CPU add / sub kernel rounds the scalar to bf16 first, so the
    plain expression is not the same function on the two devices (its mul is; the written-out form serves both)."""
    return op(x.float(), torch.tensor(value, dtype=torch.float32, device=x.device)).to(x.dtype)


def sample(mom, noise, scaling_factor, shift_factor=None):
    mean, logvar = torch.chunk(mom, 2, dim=1)
    x = mean
    if noise is not None:
        logvar = torch.clamp(logvar, -30.0, 20.0)
        std = torch.exp(0.5 * logvar)
        x = mean + std * noise.to(mom.dtype)
    if shift_factor is not None:
        x = _with_float(x, torch.sub, shift_factor)
    return _with_float(x, torch.mul, scaling_factor)


def encode(cfg, sd, images, dtype, noise=None, apply_shift=None):
    if apply_shift is None:
        apply_shift = cfg.get("shift_factor") is not None
    return sample(moments(cfg, sd, images, dtype), noise, cfg["scaling_factor"], cfg["shift_factor"] if apply_shift else None)


def random_encoder_state(cfg, seed=0, in_channels=3):
    """Random encoder weights in the diffusers layout, bf16-representable (fp32 tensors), scaled so that activations stay
    O(1) through the stack; ``conv_out`` is drawn at half scale so that the logvar half of the moments stays moderate
    (|logvar| of a few: std = exp(logvar / 2) neither vanishes nor swamps the mean)."""
    ch, n, m = list(cfg["block_out_channels"]), len(cfg["block_out_channels"]), 2 * cfg["latent_channels"]
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

    w("encoder.conv_in.weight", ch[0], in_channels, 3, 3)
    vec("encoder.conv_in.bias", ch[0])
    prev = ch[0]
    for i, c in enumerate(ch):
        for j in range(cfg["layers_per_block"]):
            res(f"encoder.down_blocks.{i}.resnets.{j}.", prev if j == 0 else c, c)
        if i < n - 1:
            w(f"encoder.down_blocks.{i}.downsamplers.0.conv.weight", c, c, 3, 3)
            vec(f"encoder.down_blocks.{i}.downsamplers.0.conv.bias", c)
        prev = c
    res("encoder.mid_block.resnets.0.", ch[-1], ch[-1])
    if cfg["mid_block_add_attention"]:
        a, c = "encoder.mid_block.attentions.0.", ch[-1]
        vec(a + "group_norm.weight", c, 1.0, 0.2)
        vec(a + "group_norm.bias", c)
        for t in ("to_q", "to_k", "to_v"):
            w(a + t + ".weight", c, c, scale=2.0)              # peaked enough that the softmax is not uniform
            vec(a + t + ".bias", c)
        w(a + "to_out.0.weight", c, c)
        vec(a + "to_out.0.bias", c)
    res("encoder.mid_block.resnets.1.", ch[-1], ch[-1])
    vec("encoder.conv_norm_out.weight", ch[-1], 1.0, 0.2)
    vec("encoder.conv_norm_out.bias", ch[-1])
    w("encoder.conv_out.weight", m, ch[-1], 3, 3, scale=0.5)
    vec("encoder.conv_out.bias", m)
    if cfg["use_post_quant_conv"]:
        w("quant_conv.weight", m, m, 1, 1)
        vec("quant_conv.bias", m)
    return sd
