"""Torch restatement of transformers' CLIPTextModelWithProjection (modeling_clip.py, eager attention), module for module and op
for op, that runs in fp32 or bf16 on any device: the reference of tests/test_clip_gpu.py (the GPU machine needs no
transformers), pinned against transformers itself in tests/test_clip_cpu.py.  One prompt at a time: the model is causal and
takes no padding mask, so a batch row is the prompt encoded alone."""
import json
import os

import torch
import torch.nn.functional as F

from tests.t5_ref import rel_l2, save_pretrained_layout  # noqa: F401  (the layout writer is model-agnostic)

E = "text_model.embeddings."


def tiny_config(act="quick_gelu", eos_token_id=2, **over):
    """hidden 128, 2 heads of 64, 3 blocks, MLP 256, projection 64, 77 positions, vocab 512."""
    cfg = dict(architectures=["CLIPTextModelWithProjection"], model_type="clip_text_model", hidden_size=128, num_hidden_layers=3,
               num_attention_heads=2, intermediate_size=256, projection_dim=64, max_position_embeddings=77, vocab_size=512,
               hidden_act=act, layer_norm_eps=1e-5, attention_dropout=0.0, bos_token_id=0, eos_token_id=eos_token_id,
               pad_token_id=1, initializer_factor=1.0, initializer_range=0.02)
    cfg.update(over)
    return cfg


def real_width_config(**over):
    """OpenCLIP bigG's widths (``text_encoder_2`` of SD3.5) at 2 blocks and a 1024-token vocabulary."""
    return tiny_config(act="gelu", hidden_size=1280, num_hidden_layers=2, num_attention_heads=20, intermediate_size=5120,
                       projection_dim=1280, vocab_size=1024, **over)


def random_state_dict(cfg, seed=0, logit_gain=1.0):
    """Seeded weights (fp32): projections ~ N(0, 1 / fan_in) with biases ~ N(0, 0.1^2), q / k weights scaled by ``logit_gain``
    (a normed row has unit scale, so a logit q . k / 8 has std about logit_gain^2), norm weights around 1 with some near 0 and
    norm biases ~ N(0, 0.1^2), token embeddings ~ N(0, 1), position embeddings ~ N(0, 0.5^2)."""
    g = torch.Generator().manual_seed(seed)
    D, Fd, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["projection_dim"]

    def lin(n, k, gain=1.0):
        return torch.randn(n, k, generator=g) * (gain / k ** 0.5)

    def vec(n, std=0.1):
        return torch.randn(n, generator=g) * std

    def norm_w():
        w = 1.0 + torch.randn(D, generator=g) * 0.2
        w[::7] -= 0.95
        return w
    sd = {E + "token_embedding.weight": torch.randn(cfg["vocab_size"], D, generator=g),
          E + "position_embedding.weight": torch.randn(cfg["max_position_embeddings"], D, generator=g) * 0.5,
          "text_model.final_layer_norm.weight": norm_w(), "text_model.final_layer_norm.bias": vec(D),
          "text_projection.weight": lin(P, D)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        for n, gain in (("q_proj", logit_gain), ("k_proj", logit_gain), ("v_proj", 1.0), ("out_proj", 1.0)):
            sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"] = lin(D, D, gain), vec(D)
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = norm_w(), vec(D)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = lin(Fd, D), vec(Fd)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = lin(D, Fd), vec(D)
    return sd


def clip_tokenizer_dir(path, pad_token):
    """vocab.json + merges.txt of a tiny byte-level BPE in CLIP's layout (all SD3.5 ships for its CLIP tokenizers), and the
    two files that name the pad token."""
    from tokenizers import pre_tokenizers
    alphabet = sorted(pre_tokenizers.ByteLevel.alphabet())
    merges = [("c", "a"), ("ca", "t</w>"), ("d", "o"), ("do", "g</w>"), ("t", "h"), ("th", "e</w>")]
    tokens = alphabet + [c + "</w>" for c in alphabet] + [a + b for a, b in merges] + ["<|startoftext|>", "<|endoftext|>"]
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "vocab.json"), "w") as f:
        json.dump({t: i for i, t in enumerate(tokens)}, f)
    with open(os.path.join(path, "merges.txt"), "w") as f:
        f.write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    special = {"bos_token": "<|startoftext|>", "eos_token": "<|endoftext|>", "unk_token": "<|endoftext|>", "pad_token": pad_token}
    with open(os.path.join(path, "special_tokens_map.json"), "w") as f:
        json.dump(special, f)
    with open(os.path.join(path, "tokenizer_config.json"), "w") as f:
        json.dump({**special, "tokenizer_class": "CLIPTokenizer", "model_max_length": 77}, f)
    return str(path)


# ---------------------------------------------------------------------------------------------------------------- modules
def quick_gelu(x):
    """QuickGELUActivation.forward, op for op (in bf16 every op rounds)."""
    return x * torch.sigmoid(1.702 * x)


def activation(name):
    return quick_gelu if name == "quick_gelu" else F.gelu             # GELUActivation: the erf form


def eager_attention(q, k, v, scale):
    """eager_attention_forward of modeling_clip.py under the causal mask: q, k, v [..., H, L, dh] -> [..., L, H * dh].  The
    mask is additive (0 / the dtype's minimum); the softmax runs in fp32 and is rounded to the query's dtype."""
    L = q.shape[-2]
    w = torch.matmul(q, k.transpose(-1, -2)) * scale
    above = torch.ones(L, L, dtype=torch.bool, device=q.device).triu(1)
    w = w + torch.zeros(L, L, dtype=q.dtype, device=q.device).masked_fill(above, torch.finfo(q.dtype).min)
    w = F.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    out = torch.matmul(w, v).transpose(-3, -2)
    return out.reshape(*out.shape[:-2], -1)


def eos_position(ids, eos_token_id):
    """CLIPTextTransformer's pooling row of ids [B, L] -> [B]."""
    if eos_token_id == 2:
        return ids.to(torch.int).argmax(dim=-1)
    return (ids.to(torch.int) == eos_token_id).int().argmax(dim=-1)


class CLIPRef:
    def __init__(self, cfg, sd, dtype=torch.float32, device="cpu"):
        self.cfg, self.dtype, self.device = cfg, dtype, device
        self.sd = {k: v.to(device, dtype) for k, v in sd.items()}

    @torch.no_grad()
    def forward(self, ids):
        """CLIPTextModelWithProjection.forward(ids [B, L], output_hidden_states=True) -> (hidden_states[-2] [B, L, hidden],
        text_embeds [B, projection_dim], last_hidden_state [B, L, hidden])."""
        c, sd = self.cfg, self.sd
        D, H, eps = c["hidden_size"], c["num_attention_heads"], c["layer_norm_eps"]
        dh, act = D // H, activation(c["hidden_act"])
        ids = ids.to(self.device)
        B, L = ids.shape
        x = F.embedding(ids, sd[E + "token_embedding.weight"]) + sd[E + "position_embedding.weight"][:L]
        states = [x]
        for i in range(c["num_hidden_layers"]):
            p = f"text_model.encoder.layers.{i}."
            a = p + "self_attn."
            h = F.layer_norm(x, (D,), sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], eps)
            q, k, v = (F.linear(h, sd[a + f"{n}_proj.weight"], sd[a + f"{n}_proj.bias"]).view(B, L, H, dh).transpose(1, 2)
                       for n in "qkv")
            x = x + F.linear(eager_attention(q, k, v, dh ** -0.5), sd[a + "out_proj.weight"], sd[a + "out_proj.bias"])
            h = F.layer_norm(x, (D,), sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], eps)
            h = act(F.linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
            x = x + F.linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
            states.append(x)
        last = F.layer_norm(x, (D,), sd["text_model.final_layer_norm.weight"], sd["text_model.final_layer_norm.bias"], eps)
        pooled = last[torch.arange(B, device=self.device), eos_position(ids, c["eos_token_id"])]
        return states[-2], F.linear(pooled, sd["text_projection.weight"]), last

    def encode(self, prompts, max_batch=None):
        """One prompt at a time: ids list -> list of (hidden_states[-2] [L_i, hidden], text_embeds [projection_dim])."""
        out = []
        for p in prompts:
            hs, te, _ = self.forward(torch.as_tensor(p).reshape(1, -1).long())
            out.append((hs[0], te[0]))
        return out
