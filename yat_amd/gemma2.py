"""Gemma-2 text encoder on the HIP kernels: the ``text_encoder`` of a SANA pipeline directory (transformers ``Gemma2Model``;
``pipe.encode_prompt`` at train_sana.py:84-94,113-129 and common/trainer.py:307-308), forward only, bf16.

The text side runs packed: ``encode`` takes the prompts' token ids as a list of 1-D tensors, lays them end to end as the rows
of one matrix and computes no pad row.  That is exact, not an approximation: the reference pads on the right and the model is
causal, so a real token never attends to a pad (a right-padded batch and the same prompt alone agree to the bit in fp32
transformers on the real rows).

Per block (Gemma2DecoderLayer): input_layernorm -> q|k|v projection (one GEMM) -> RoPE -> attention -> o_proj ->
post_attention_layernorm + residual add (one kernel) -> pre_feedforward_layernorm -> gate|up projection (one GEMM) -> GeGLU ->
down_proj -> post_feedforward_layernorm + residual add; then the final ``norm``.  Rounding points are those of the bf16
module: one per torch op (include/yat_hip.h, "Gemma-2 text encoder").  The GeGLU is its own row kernel: the GEMM epilogue's
gate multiply takes the unrounded up_proj accumulator, the module rounds it first.

Soft cap.  ``config.attn_logit_softcapping`` (50 in Gemma-2) is part of the model as defined and trained, and transformers'
eager attention applies it; ``softcap=True`` (the default) follows the config.  transformers' SDPA attention path -- the
default of recent versions -- silently drops the cap, so which form a given diffusers / transformers install computes
depends on its versions; ``softcap=False`` reproduces that form.  ``describe()`` names the form that runs.

Sliding window.  Below ``sliding_window`` tokens Gemma-2's sliding layers equal its full layers; a prompt longer than
``min(sliding_window, max_position_embeddings, 1024)`` is refused (SANA uses at most a few hundred tokens).
"""
from __future__ import annotations

import torch

from .text_common import TextEncoderHIP, read_text_encoder_tensors
from .vae_common import BF16, check_expected, read_config

MAX_PROMPT = 1024                     # yat_gemma_attn_fwd's bound on one prompt

_NORMS = ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm")


def rope_theta(cfg: dict) -> float:
    rp = cfg.get("rope_parameters") or {}
    return float(cfg.get("rope_theta") or rp.get("rope_theta") or 10000.0)


def validate_config(cfg: dict) -> None:
    """Refuse what the kernels do not compute."""
    if cfg.get("hidden_activation", "gelu_pytorch_tanh") != "gelu_pytorch_tanh":
        raise NotImplementedError(f"Gemma-2 hidden_activation {cfg.get('hidden_activation')!r}: only gelu_pytorch_tanh is built")
    if cfg.get("attention_bias", False):
        raise NotImplementedError("Gemma-2 attention_bias = true is not built (the projections have no bias)")
    if int(cfg.get("head_dim", 0)) != 256:
        raise NotImplementedError(f"Gemma-2 head_dim {cfg.get('head_dim')}: the attention kernel is built for 256")
    if int(cfg["num_attention_heads"]) % int(cfg["num_key_value_heads"]):
        raise ValueError("num_attention_heads must be a multiple of num_key_value_heads")
    if int(cfg["hidden_size"]) % 8 or int(cfg["intermediate_size"]) % 8:
        raise NotImplementedError("hidden_size and intermediate_size must be multiples of 8")
    rtype = (cfg.get("rope_parameters") or {}).get("rope_type", "default")
    if rtype != "default" or cfg.get("rope_scaling"):
        raise NotImplementedError("only the default rotary embedding is built")


def expected_keys(cfg: dict) -> dict:
    """{key (without the ``model.`` prefix): shape} of a Gemma2Model state dict."""
    H, I, dh = int(cfg["hidden_size"]), int(cfg["intermediate_size"]), int(cfg["head_dim"])
    Hq, Hkv = int(cfg["num_attention_heads"]), int(cfg["num_key_value_heads"])
    want = {"embed_tokens.weight": (int(cfg["vocab_size"]), H), "norm.weight": (H,)}
    for i in range(int(cfg["num_hidden_layers"])):
        p = f"layers.{i}."
        want[p + "self_attn.q_proj.weight"] = (Hq * dh, H)
        want[p + "self_attn.k_proj.weight"] = (Hkv * dh, H)
        want[p + "self_attn.v_proj.weight"] = (Hkv * dh, H)
        want[p + "self_attn.o_proj.weight"] = (H, Hq * dh)
        want[p + "mlp.gate_proj.weight"] = (I, H)
        want[p + "mlp.up_proj.weight"] = (I, H)
        want[p + "mlp.down_proj.weight"] = (H, I)
        for n in _NORMS:
            want[p + n + ".weight"] = (H,)
    return want


def _stored_key(k: str):
    kk = k[len("model."):] if k.startswith("model.") else k
    return None if kk.startswith("lm_head.") else kk


def load_text_encoder_dir(te_dir: str):
    """A transformers Gemma-2 directory -> (config dict, {key without ``model.``: tensor}).  Reads ``model.safetensors`` or
    the shards of ``model.safetensors.index.json``; ``lm_head.*`` is ignored; a missing or unexpected key raises and names it."""
    cfg = read_config(te_dir)
    validate_config(cfg)
    sd = read_text_encoder_tensors(te_dir, _stored_key)
    check_expected(expected_keys(cfg), sd, lambda k: True, "Gemma-2", "Gemma2EncoderHIP")
    return cfg, sd


def rope_tables(dh: int, theta: float, length: int, dtype=BF16):
    """cos / sin ``[length, dh]`` exactly as Gemma2RotaryEmbedding builds them: fp32 angles, then the cast."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float) / dh))
    freqs = torch.arange(length, dtype=torch.float)[:, None] * inv_freq[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


class Gemma2EncoderHIP(TextEncoderHIP):
    """Host side of the Gemma-2 encoder: packed weights on the device and the activation buffers of the largest call."""
    model_type = "gemma2"
    load_text_encoder_dir = staticmethod(load_text_encoder_dir)
    EMPTY_HINT = "the tokenizer's template supplies BOS"
    MAX_PROMPT_RULE = "min(sliding_window, max_position_embeddings, 1024)"

    def __init__(self, cfg: dict, sd: dict, device="cuda", softcap: bool = True):
        validate_config(cfg)
        super().__init__(cfg, device)
        self.H, self.I, self.dh = int(cfg["hidden_size"]), int(cfg["intermediate_size"]), int(cfg["head_dim"])
        self.Hq, self.Hkv = int(cfg["num_attention_heads"]), int(cfg["num_key_value_heads"])
        self.L = int(cfg["num_hidden_layers"])
        self.eps = float(cfg.get("rms_norm_eps", 1e-6))
        self.scale = float(cfg.get("query_pre_attn_scalar", self.dh)) ** -0.5
        cap = cfg.get("attn_logit_softcapping")
        self.softcap = float(cap) if (softcap and cap) else 0.0
        self.max_prompt = min(int(cfg.get("sliding_window") or MAX_PROMPT), int(cfg.get("max_position_embeddings") or MAX_PROMPT),
                              MAX_PROMPT)
        self.embed_scale = float(torch.tensor(self.H ** 0.5).to(BF16))          # embed_scale.to(weight.dtype)
        dev = self.dev
        self.embed = dev(sd["embed_tokens.weight"])
        self.norm = dev(sd["norm.weight"])
        self.layers = []
        for i in range(self.L):
            p = f"layers.{i}."
            a = p + "self_attn."
            self.layers.append({
                "qkv": dev(torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]], 0)),
                "o": dev(sd[a + "o_proj.weight"]),
                "gu": dev(torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], 0)),
                "down": dev(sd[p + "mlp.down_proj.weight"]),
                **{n: dev(sd[p + n + ".weight"]) for n in _NORMS}})
        cos, sin = rope_tables(self.dh, rope_theta(cfg), self.max_prompt)
        self.cos, self.sin = cos.to(self.device), sin.to(self.device)

    def describe(self) -> str:
        cap = self.cfg.get("attn_logit_softcapping")
        form = (f"attention logits soft-capped at {self.softcap:g} (the model as defined; transformers' eager attention)"
                if self.softcap else
                f"attention logits NOT soft-capped (config: {cap}; the form transformers' SDPA attention computes)")
        return f"Gemma-2 text encoder on HIP: {self.L} layers, hidden {self.H}, {self.Hq}/{self.Hkv} heads of {self.dh}; {form}"

    def _buffer_widths(self):
        return {"h": self.H, "n": self.H, "qkv": (self.Hq + 2 * self.Hkv) * self.dh, "a": self.Hq * self.dh, "gu": 2 * self.I,
                "act": self.I}

    def _forward(self, pack, bufs, y):
        from . import ops
        ids, off_d, lens, rows, B = pack.ids, pack.off_d, pack.lens, pack.rows, len(pack.lens)
        pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).to(self.device)
        h, n, qkv, a, gu, act = (bufs[k] for k in ("h", "n", "qkv", "a", "gu", "act"))
        H, I, dh, Hq, Hkv = self.H, self.I, self.dh, self.Hq, self.Hkv
        ops.embed_rows(ids, self.embed, self.embed_scale, h)
        for w in self.layers:
            ops.gemma_rmsnorm(h, w["input_layernorm"], n, self.eps)
            ops.gemm(n, w["qkv"], qkv, M=rows, N=qkv.shape[1], K=H)
            ops.rope_qk(qkv, Hq + Hkv, dh, pos, self.cos, self.sin)
            ops.gemma_attn_fwd(qkv, off_d, B, Hq, Hkv, dh, max(lens), self.scale, self.softcap, a)
            ops.gemm(a, w["o"], n, M=rows, N=H, K=Hq * dh)
            ops.gemma_rmsnorm(n, w["post_attention_layernorm"], h, self.eps, residual=h)
            ops.gemma_rmsnorm(h, w["pre_feedforward_layernorm"], n, self.eps)
            ops.gemm(n, w["gu"], gu, M=rows, N=2 * I, K=H)
            ops.geglu(gu, I, act)
            ops.gemm(act, w["down"], n, M=rows, N=H, K=I)
            ops.gemma_rmsnorm(n, w["post_feedforward_layernorm"], h, self.eps, residual=h)
        ops.gemma_rmsnorm(h, self.norm, y, self.eps)
