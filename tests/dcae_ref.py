"""Torch restatement of the diffusers AutoencoderDC decoder [RECALL] for the DC-AE tests, written apart from yat_amd/dcae.py
(it does not import yat_amd).  NCHW, weights in the diffusers key layout (``decoder.*``), on any torch device.

    decode(cfg, sd, latent, dtype)   dtype = torch.bfloat16: the reference's bf16 VAE, every module output rounded
                                     dtype = torch.float32:  the same weights in fp32 arithmetic (the ground truth)

``cfg`` is a plain dict: latent_channels, block_out_channels, block_types, layers_per_block, scaling_factor (per-stage
values as lists; SANA's qkv_multiscales (5,), head dim 32 and rms_norm / silu are the only forms restated here).
"""
import torch
import torch.nn.functional as F

EPS = 1e-5


def rms_norm(x, w, b):
    """diffusers RMSNorm over the channel dim of an NCHW tensor (movedim(1, -1) ... movedim(-1, 1))."""
    h = x.movedim(1, -1)
    var = h.to(torch.float32).pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(var + EPS)
    if w.dtype in (torch.float16, torch.bfloat16):
        h = h.to(w.dtype)
    h = h * w
    h = h + b
    return h.movedim(-1, 1)


def conv(x, w, b=None, pad=1, groups=1):
    return F.conv2d(x, w, b, padding=pad, groups=groups)


def res_block(x, sd, p):
    h = F.silu(conv(x, sd[p + "conv1.weight"], sd[p + "conv1.bias"]))
    h = conv(h, sd[p + "conv2.weight"])
    return rms_norm(h, sd[p + "norm.weight"], sd[p + "norm.bias"]) + x


def linear_attention(q, k, v, eps=1e-15):
    v = F.pad(v, (0, 0, 0, 1), mode="constant", value=1)
    scores = torch.matmul(v, k.transpose(-1, -2))
    h = torch.matmul(scores, q).to(torch.float32)
    return h[:, :, :-1] / (h[:, :, -1:] + eps)


def msla_processor(x, sd, a, head_dim=32):
    """SanaMultiscaleAttnProcessor2_0 up to (excluding) to_out: [B, C, H, W] -> [B, 2C, H, W]."""
    B, C, H, W = x.shape
    if H * W <= head_dim:
        raise ValueError("quadratic form not restated")
    hs = x.movedim(1, -1)
    qkv = torch.cat([F.linear(hs, sd[a + "to_q.weight"]), F.linear(hs, sd[a + "to_k.weight"]),
                     F.linear(hs, sd[a + "to_v.weight"])], dim=3).movedim(-1, 1)
    c3 = qkv.shape[1]
    agg = conv(qkv, sd[a + "to_qkv_multiscale.0.proj_in.weight"], pad=2, groups=c3)
    agg = conv(agg, sd[a + "to_qkv_multiscale.0.proj_out.weight"], pad=0, groups=c3 // head_dim)
    dtype = qkv.dtype
    h = torch.cat([qkv, agg], dim=1).to(torch.float32)
    h = h.reshape(B, -1, 3 * head_dim, H * W)
    q, k, v = h.chunk(3, dim=2)
    q, k = F.relu(q), F.relu(k)
    h = linear_attention(q, k, v).to(dtype)
    return torch.reshape(h, (B, -1, H, W))


def evit_block(x, sd, p):
    a = p + "attn."
    h = msla_processor(x, sd, a)
    h = F.linear(h.movedim(1, -1), sd[a + "to_out.weight"]).movedim(-1, 1)
    x = rms_norm(h, sd[a + "norm_out.weight"], sd[a + "norm_out.bias"]) + x
    g = p + "conv_out."
    h = F.silu(conv(x, sd[g + "conv_inverted.weight"], sd[g + "conv_inverted.bias"], pad=0))
    h = conv(h, sd[g + "conv_depth.weight"], sd[g + "conv_depth.bias"], pad=1, groups=h.shape[1])
    h, gate = torch.chunk(h, 2, dim=1)
    h = h * F.silu(gate)
    h = conv(h, sd[g + "conv_point.weight"], pad=0)
    return rms_norm(h, sd[g + "norm.weight"], sd[g + "norm.bias"]) + x


def up_block(x, sd, p, c_out):
    y = F.interpolate(x, scale_factor=2, mode="nearest")
    y = conv(y, sd[p + "conv.weight"], sd[p + "conv.bias"])
    r = c_out * 4 // x.shape[1]
    s = F.pixel_shuffle(x.repeat_interleave(r, dim=1), 2)
    return y + s


def decode(cfg, sd, latent, dtype):
    sd = {k: v.to(latent.device, dtype) for k, v in sd.items() if k.startswith("decoder.")}
    ch, n = list(cfg["block_out_channels"]), len(cfg["block_out_channels"])
    z = (latent.float() / cfg["scaling_factor"]).to(dtype)
    x = conv(z, sd["decoder.conv_in.weight"], sd["decoder.conv_in.bias"]) + z.repeat_interleave(ch[-1] // z.shape[1], dim=1)
    for i in reversed(range(n)):
        j = 0
        if i < n - 1:
            x = up_block(x, sd, f"decoder.up_blocks.{i}.0.", ch[i])
            j = 1
        for jj in range(j, j + cfg["layers_per_block"][i]):
            p = f"decoder.up_blocks.{i}.{jj}."
            x = res_block(x, sd, p) if cfg["block_types"][i] == "ResBlock" else evit_block(x, sd, p)
    x = F.relu(rms_norm(x, sd["decoder.norm_out.weight"], sd["decoder.norm_out.bias"]))
    return conv(x, sd["decoder.conv_out.weight"], sd["decoder.conv_out.bias"])


def postprocess(x):
    """VaeImageProcessor.postprocess (denormalize in the tensor's dtype) + numpy_to_pil's uint8: [B, 3, H, W] -> uint8."""
    p = (x / 2 + 0.5).clamp(0, 1)
    return (p.cpu().float() * 255).numpy().round().astype("uint8")


def weight_drawers(seed):
    """(sd, w, vec): ``w(key, *shape, scale=1.0)`` draws a weight of std scale / sqrt(fan-in) into ``sd``, ``vec(key, c, mean,
    std)`` a vector, both bf16-representable fp32 tensors from one generator seeded ``seed``."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def w(k, *shape, scale=1.0):
        fan = shape[1] * (shape[2] * shape[3] if len(shape) == 4 else 1)
        sd[k] = (torch.randn(*shape, generator=g) * (scale / fan ** 0.5)).to(torch.bfloat16).float()

    def vec(k, c, mean=0.0, std=0.1):
        sd[k] = (mean + std * torch.randn(c, generator=g)).to(torch.bfloat16).float()

    return sd, w, vec


def random_block(w, vec, p, block_type, c):
    """Draws the weights of one ResBlock / EfficientViTBlock of width ``c`` under the prefix ``p``."""
    if block_type == "ResBlock":
        w(p + "conv1.weight", c, c, 3, 3)
        vec(p + "conv1.bias", c)
        w(p + "conv2.weight", c, c, 3, 3)
        vec(p + "norm.weight", c, 1.0, 0.2)
        vec(p + "norm.bias", c)
        return
    a = p + "attn."
    for t in ("to_q", "to_k", "to_v"):
        w(a + t + ".weight", c, c)
    w(a + "to_qkv_multiscale.0.proj_in.weight", 3 * c, 1, 5, 5)
    w(a + "to_qkv_multiscale.0.proj_out.weight", 3 * c, 32, 1, 1)
    w(a + "to_out.weight", c, 2 * c)
    vec(a + "norm_out.weight", c, 1.0, 0.2)
    vec(a + "norm_out.bias", c)
    gg = p + "conv_out."
    w(gg + "conv_inverted.weight", 8 * c, c, 1, 1)
    vec(gg + "conv_inverted.bias", 8 * c)
    w(gg + "conv_depth.weight", 8 * c, 1, 3, 3)
    vec(gg + "conv_depth.bias", 8 * c)
    w(gg + "conv_point.weight", c, 4 * c, 1, 1)
    vec(gg + "norm.weight", c, 1.0, 0.2)
    vec(gg + "norm.bias", c)


def random_state(cfg, seed=0, out_channels=3):
    """Random decoder weights in the diffusers layout, bf16-representable (fp32 tensors), scaled so that activations stay
    O(1) through the stack."""
    ch, n, lat = list(cfg["block_out_channels"]), len(cfg["block_out_channels"]), cfg["latent_channels"]
    sd, w, vec = weight_drawers(seed)
    w("decoder.conv_in.weight", ch[-1], lat, 3, 3)
    vec("decoder.conv_in.bias", ch[-1])
    for i in range(n):
        c, j = ch[i], 0
        if i < n - 1:
            w(f"decoder.up_blocks.{i}.0.conv.weight", c, ch[i + 1], 3, 3)
            vec(f"decoder.up_blocks.{i}.0.conv.bias", c)
            j = 1
        for jj in range(j, j + cfg["layers_per_block"][i]):
            random_block(w, vec, f"decoder.up_blocks.{i}.{jj}.", cfg["block_types"][i], c)
    vec("decoder.norm_out.weight", ch[0], 1.0, 0.2)
    vec("decoder.norm_out.bias", ch[0])
    w("decoder.conv_out.weight", out_channels, ch[0], 3, 3)
    vec("decoder.conv_out.bias", out_channels)
    return sd


def diffusers_config(cfg):
    """The ``vae/config.json`` of an AutoencoderDC with this decoder (list forms of the per-stage keys)."""
    n = len(cfg["block_out_channels"])
    return {"_class_name": "AutoencoderDC", "in_channels": 3, "latent_channels": cfg["latent_channels"],
            "attention_head_dim": 32, "decoder_block_types": list(cfg["block_types"]),
            "decoder_block_out_channels": list(cfg["block_out_channels"]),
            "decoder_layers_per_block": list(cfg["layers_per_block"]),
            "decoder_qkv_multiscales": [[5] if t == "EfficientViTBlock" else [] for t in cfg["block_types"]],
            "decoder_norm_types": ["rms_norm"] * n, "decoder_act_fns": ["silu"] * n,
            "upsample_block_type": "interpolate", "scaling_factor": cfg["scaling_factor"]}


SANA_F32C32 = {"latent_channels": 32, "block_out_channels": [128, 256, 512, 512, 1024, 1024],
               "block_types": ["ResBlock"] * 3 + ["EfficientViTBlock"] * 3, "layers_per_block": [3] * 6,
               "scaling_factor": 0.41407}
