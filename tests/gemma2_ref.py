"""Torch restatement of transformers' Gemma2Model (modeling_gemma2.py, eager attention), module for module and op for op, that
runs in fp32 or bf16 on any device: the reference of tests/test_gemma2_gpu.py (the GPU machine needs no transformers), pinned
against transformers itself in tests/test_gemma2_cpu.py.  One prompt at a time, without padding: the model is causal and the
pipeline pads on the right, so that is what the real rows of a padded batch see."""
import json
import os

import torch
import torch.nn.functional as F

NORMS = ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm")


def tiny_config(**over):
    """The small config of the issue: hidden 256, 3 layers, 2 / 1 heads of 256, MLP 512, vocab 512."""
    cfg = dict(architectures=["Gemma2Model"], model_type="gemma2", hidden_size=256, num_hidden_layers=3, num_attention_heads=2,
               num_key_value_heads=1, head_dim=256, intermediate_size=512, vocab_size=512, rms_norm_eps=1e-6,
               query_pre_attn_scalar=256, attn_logit_softcapping=50.0, final_logit_softcapping=30.0, sliding_window=4096,
               max_position_embeddings=8192, hidden_activation="gelu_pytorch_tanh", attention_bias=False, rope_theta=10000.0)
    cfg.update(over)
    return cfg


def real_width_config(**over):
    """Gemma-2-2B's widths at 2 layers and a 1024-token vocabulary."""
    return tiny_config(hidden_size=2304, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=4,
                       intermediate_size=9216, vocab_size=1024, **over)


def random_state_dict(cfg, seed=0, logit_gain=1.0):
    """Seeded weights (fp32): projections ~ N(0, 1 / fan_in), q / k scaled by ``logit_gain`` (to push the pre-cap logits),
    norm weights around 0 with some near -1, embeddings ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    H, I, dh = cfg["hidden_size"], cfg["intermediate_size"], cfg["head_dim"]
    Hq, Hkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]

    def lin(n, k, gain=1.0):
        return torch.randn(n, k, generator=g) * (gain / k ** 0.5)

    def norm_w():
        w = torch.randn(H, generator=g) * 0.2
        w[::7] -= 0.9
        return w
    sd = {"embed_tokens.weight": torch.randn(cfg["vocab_size"], H, generator=g), "norm.weight": norm_w()}
    for i in range(cfg["num_hidden_layers"]):
        p = f"layers.{i}."
        sd[p + "self_attn.q_proj.weight"] = lin(Hq * dh, H, logit_gain)
        sd[p + "self_attn.k_proj.weight"] = lin(Hkv * dh, H, logit_gain)
        sd[p + "self_attn.v_proj.weight"] = lin(Hkv * dh, H)
        sd[p + "self_attn.o_proj.weight"] = lin(H, Hq * dh)
        sd[p + "mlp.gate_proj.weight"] = lin(I, H)
        sd[p + "mlp.up_proj.weight"] = lin(I, H)
        sd[p + "mlp.down_proj.weight"] = lin(H, I)
        for n in NORMS:
            sd[p + n + ".weight"] = norm_w()
    return sd


def save_pretrained_layout(te_dir, cfg, sd, prefix="", shards=1, extra=None):
    """What ``save_pretrained`` leaves: config.json + model.safetensors, or ``shards`` files + model.safetensors.index.json."""
    from safetensors.torch import save_file
    os.makedirs(te_dir, exist_ok=True)
    with open(os.path.join(te_dir, "config.json"), "w") as f:
        json.dump(cfg, f)
    full = {prefix + k: v.contiguous() for k, v in sd.items()}
    full.update(extra or {})
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
def rmsnorm(x, w, eps):
    """Gemma2RMSNorm.forward."""
    out = x.float()
    out = out * torch.rsqrt(out.pow(2).mean(-1, keepdim=True) + eps)
    out = out * (1.0 + w.float())
    return out.type_as(x)


def rope_tables(dh, theta, length, dtype):
    """Gemma2RotaryEmbedding.forward for positions 0 .. length - 1: fp32 angles, then the cast."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float) / dh))
    freqs = torch.arange(length, dtype=torch.float)[:, None] * inv_freq[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def apply_rope(x, cos, sin):
    """apply_rotary_pos_emb for one of q / k: x [..., heads, L, dh], cos / sin [L, dh]."""
    return (x * cos) + (rotate_half(x) * sin)


def eager_attention(q, k, v, scale, softcap, key_mask=None):
    """eager_attention_forward with the causal (and key padding) mask: q [..., Hq, L, dh], k / v [..., Hkv, L, dh] -> [..., L,
    Hq * dh].  ``key_mask``: [B, L] (1 = real token) for a batched, right-padded call."""
    G, L = q.shape[-3] // k.shape[-3], q.shape[-2]
    k, v = k.repeat_interleave(G, -3), v.repeat_interleave(G, -3)                   # repeat_kv
    w = torch.matmul(q, k.transpose(-1, -2)) * scale
    if softcap:
        w = w / softcap
        w = torch.tanh(w)
        w = w * softcap
    allowed = torch.ones(L, L, dtype=torch.bool, device=q.device).tril()
    if key_mask is not None:
        allowed = allowed[None, None] & key_mask.bool().to(q.device)[:, None, None, :]
    w = w + torch.zeros_like(w).masked_fill(~allowed, torch.finfo(q.dtype).min)
    w = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    out = torch.matmul(w, v).transpose(-3, -2)
    return out.reshape(*out.shape[:-2], -1)


class Gemma2Ref:
    def __init__(self, cfg, sd, dtype=torch.float32, device="cpu", softcap=True):
        self.cfg, self.dtype, self.device = cfg, dtype, device
        self.sd = {(k[6:] if k.startswith("model.") else k): v.to(device, dtype) for k, v in sd.items()}
        self.softcap = cfg.get("attn_logit_softcapping") if softcap else None
        self.theta = float(cfg.get("rope_theta") or (cfg.get("rope_parameters") or {}).get("rope_theta") or 10000.0)

    @torch.no_grad()
    def forward(self, ids, attention_mask=None):
        """Gemma2Model.forward: ids [B, L] (right-padded, with ``attention_mask`` [B, L]) -> last_hidden_state [B, L, hidden]."""
        c, sd = self.cfg, self.sd
        H, dh, Hq, Hkv, eps = c["hidden_size"], c["head_dim"], c["num_attention_heads"], c["num_key_value_heads"], c["rms_norm_eps"]
        B, L = ids.shape
        x = F.embedding(ids.to(self.device), sd["embed_tokens.weight"]) * torch.tensor(H ** 0.5).to(self.dtype)
        cos, sin = (t.to(self.device) for t in rope_tables(dh, self.theta, L, self.dtype))
        for i in range(c["num_hidden_layers"]):
            p = f"layers.{i}."
            a = p + "self_attn."
            res = x
            h = rmsnorm(x, sd[p + "input_layernorm.weight"], eps)
            q = F.linear(h, sd[a + "q_proj.weight"]).view(B, L, Hq, dh).transpose(1, 2)
            k = F.linear(h, sd[a + "k_proj.weight"]).view(B, L, Hkv, dh).transpose(1, 2)
            v = F.linear(h, sd[a + "v_proj.weight"]).view(B, L, Hkv, dh).transpose(1, 2)
            q, k = apply_rope(q, cos, sin), apply_rope(k, cos, sin)
            h = eager_attention(q, k, v, c["query_pre_attn_scalar"] ** -0.5, self.softcap, attention_mask)
            h = F.linear(h, sd[a + "o_proj.weight"])
            x = res + rmsnorm(h, sd[p + "post_attention_layernorm.weight"], eps)
            res = x
            h = rmsnorm(x, sd[p + "pre_feedforward_layernorm.weight"], eps)
            h = F.linear(F.gelu(F.linear(h, sd[p + "mlp.gate_proj.weight"]), approximate="tanh") *
                         F.linear(h, sd[p + "mlp.up_proj.weight"]), sd[p + "mlp.down_proj.weight"])
            x = res + rmsnorm(h, sd[p + "post_feedforward_layernorm.weight"], eps)
        return rmsnorm(x, sd["norm.weight"], eps)

    def encode(self, prompts, max_batch=None):
        """One prompt at a time, unpadded: ids list -> list of [L_i, hidden]."""
        return [self.forward(torch.as_tensor(p).reshape(1, -1).long())[0] for p in prompts]


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()
