"""Torch restatement of transformers' T5EncoderModel (modeling_t5.py, eager attention), module for module and op for op, that
runs in fp32 or bf16 on any device: the reference of tests/test_t5_gpu.py (the GPU machine needs no transformers), pinned
against transformers itself in tests/test_t5_cpu.py.  One prompt at a time, without padding: the pipeline pads on the right,
pad keys are masked and the position bias depends on the distance only, so that is what the real rows of a padded batch see."""
import json
import math
import os

import torch
import torch.nn.functional as F

REL = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def tiny_config(**over):
    """d_model 128, 2 blocks, 4 heads of 64, d_ff 256, vocab 512."""
    cfg = dict(architectures=["T5EncoderModel"], model_type="t5", d_model=128, num_layers=2, num_heads=4, d_kv=64, d_ff=256,
               vocab_size=512, layer_norm_epsilon=1e-6, relative_attention_num_buckets=32, relative_attention_max_distance=128,
               feed_forward_proj="gated-gelu", dense_act_fn="gelu_new", is_gated_act=True, is_encoder_decoder=False,
               is_decoder=False, tie_word_embeddings=False, dropout_rate=0.1, n_positions=512)
    cfg.update(over)
    return cfg


def real_width_config(**over):
    """T5-XXL's widths (the text encoder of PixArt-Sigma) at 1 block and a 1024-token vocabulary."""
    return tiny_config(d_model=4096, num_layers=1, num_heads=64, d_ff=10240, vocab_size=1024, **over)


def random_state_dict(cfg, seed=0, logit_gain=1.0):
    """Seeded weights (fp32): projections ~ N(0, 1 / fan_in), q / k scaled by ``logit_gain`` (T5 has no 1 / sqrt(dh): with norm
    weights around 1 a logit has std 8 * logit_gain^2), norm weights around 1 with some near 0, the relative-position bias
    ~ N(0, 3^2), embeddings ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    D, Fd, dh, H = cfg["d_model"], cfg["d_ff"], cfg["d_kv"], cfg["num_heads"]

    def lin(n, k, gain=1.0):
        return torch.randn(n, k, generator=g) * (gain / k ** 0.5)

    def norm_w():
        w = 1.0 + torch.randn(D, generator=g) * 0.2
        w[::7] -= 0.95
        return w
    sd = {"shared.weight": torch.randn(cfg["vocab_size"], D, generator=g), "encoder.final_layer_norm.weight": norm_w(),
          REL: torch.randn(cfg["relative_attention_num_buckets"], H, generator=g) * 3.0}
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}."
        a, f = p + "layer.0.SelfAttention.", p + "layer.1.DenseReluDense."
        sd[a + "q.weight"] = lin(H * dh, D, logit_gain)
        sd[a + "k.weight"] = lin(H * dh, D, logit_gain)
        sd[a + "v.weight"] = lin(H * dh, D)
        sd[a + "o.weight"] = lin(D, H * dh)
        sd[f + "wi_0.weight"] = lin(Fd, D)
        sd[f + "wi_1.weight"] = lin(Fd, D)
        sd[f + "wo.weight"] = lin(D, Fd)
        sd[p + "layer.0.layer_norm.weight"] = norm_w()
        sd[p + "layer.1.layer_norm.weight"] = norm_w()
    return sd


def save_pretrained_layout(te_dir, cfg, sd, shards=1, extra=None):
    """What ``save_pretrained`` leaves: config.json + model.safetensors, or ``shards`` files + model.safetensors.index.json."""
    from safetensors.torch import save_file
    os.makedirs(te_dir, exist_ok=True)
    with open(os.path.join(te_dir, "config.json"), "w") as f:
        json.dump(cfg, f)
    full = {k: v.contiguous() for k, v in sd.items()}
    full.update(extra or {})
    for name in os.listdir(te_dir):                                  # a rewrite in another layout leaves no stale file
        if name.endswith(".safetensors") or name.endswith(".index.json"):
            os.remove(os.path.join(te_dir, name))
    if shards == 1:
        save_file(full, os.path.join(te_dir, "model.safetensors"))
        return
    keys = sorted(full)
    weight_map = {}
    for s in range(shards):
        name = f"model-{s + 1:05d}-of-{shards:05d}.safetensors"
        part = {k: full[k] for k in keys[s::shards]}
        save_file(part, os.path.join(te_dir, name))
        weight_map.update({k: name for k in part})
    with open(os.path.join(te_dir, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {}, "weight_map": weight_map}, f)


# ---------------------------------------------------------------------------------------------------------------- modules
def layer_norm(x, w, eps):
    """T5LayerNorm.forward: fp32 variance, the product rounded to the weight's dtype, then the weight."""
    variance = x.to(torch.float32).pow(2).mean(-1, keepdim=True)
    x = x * torch.rsqrt(variance + eps)
    if w.dtype in (torch.float16, torch.bfloat16):
        x = x.to(w.dtype)
    return w * x


def gelu_new(x):
    """NewGELUActivation.forward, op for op (in bf16 every op rounds)."""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket(bidirectional=True)."""
    num_buckets //= 2
    buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    if_large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact)
                            * (num_buckets - max_exact)).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, num_buckets - 1))
    return buckets + torch.where(is_small, relative_position, if_large)


def compute_bias(weight, L, num_buckets=32, max_distance=128):
    """T5Attention.compute_bias(L, L) -> [1, H, L, L]."""
    ctx = torch.arange(L, dtype=torch.long, device=weight.device)[:, None]
    mem = torch.arange(L, dtype=torch.long, device=weight.device)[None, :]
    values = F.embedding(relative_position_bucket(mem - ctx, num_buckets, max_distance), weight)
    return values.permute([2, 0, 1]).unsqueeze(0)


def eager_attention(q, k, v, position_bias, key_mask=None):
    """eager_attention_forward of modeling_t5.py with scaling 1: q, k, v [..., H, L, dh], position_bias [1, H, L, L] (or
    [H, L, L]) -> [..., L, H * dh].  ``key_mask``: [B, L] (1 = real token) for a batched, right-padded call."""
    w = torch.matmul(q, k.transpose(-1, -2)) * 1.0
    w = w + position_bias
    if key_mask is not None:
        allowed = key_mask.bool().to(q.device)[:, None, None, :]
        w = w + torch.zeros(allowed.shape, dtype=q.dtype, device=q.device).masked_fill(~allowed, torch.finfo(q.dtype).min)
    w = F.softmax(w, dim=-1)
    out = torch.matmul(w, v).transpose(-3, -2)
    return out.reshape(*out.shape[:-2], -1)


class T5Ref:
    def __init__(self, cfg, sd, dtype=torch.float32, device="cpu"):
        self.cfg, self.dtype, self.device = cfg, dtype, device
        self.sd = {k: v.to(device, dtype) for k, v in sd.items()}
        if "shared.weight" not in self.sd:
            self.sd["shared.weight"] = self.sd["encoder.embed_tokens.weight"]

    @torch.no_grad()
    def forward(self, ids, attention_mask=None):
        """T5EncoderModel.forward: ids [B, L] (right-padded, with ``attention_mask`` [B, L]) -> last_hidden_state [B, L, d_model]."""
        c, sd = self.cfg, self.sd
        H, dh, eps = c["num_heads"], c["d_kv"], c["layer_norm_epsilon"]
        B, L = ids.shape
        x = F.embedding(ids.to(self.device), sd["shared.weight"])
        bias = compute_bias(sd[REL], L, c["relative_attention_num_buckets"], c["relative_attention_max_distance"])
        for i in range(c["num_layers"]):
            p = f"encoder.block.{i}."
            a, f = p + "layer.0.SelfAttention.", p + "layer.1.DenseReluDense."
            h = layer_norm(x, sd[p + "layer.0.layer_norm.weight"], eps)
            q = F.linear(h, sd[a + "q.weight"]).view(B, L, H, dh).transpose(1, 2)
            k = F.linear(h, sd[a + "k.weight"]).view(B, L, H, dh).transpose(1, 2)
            v = F.linear(h, sd[a + "v.weight"]).view(B, L, H, dh).transpose(1, 2)
            x = x + F.linear(eager_attention(q, k, v, bias, attention_mask), sd[a + "o.weight"])
            h = layer_norm(x, sd[p + "layer.1.layer_norm.weight"], eps)
            x = x + F.linear(gelu_new(F.linear(h, sd[f + "wi_0.weight"])) * F.linear(h, sd[f + "wi_1.weight"]), sd[f + "wo.weight"])
        return layer_norm(x, sd["encoder.final_layer_norm.weight"], eps)

    def encode(self, prompts, max_batch=None):
        """One prompt at a time, unpadded: ids list -> list of [L_i, d_model]."""
        return [self.forward(torch.as_tensor(p).reshape(1, -1).long())[0] for p in prompts]


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()
