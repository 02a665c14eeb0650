"""T5 v1.1 encoder on the HIP kernels: the ``text_encoder`` of a PixArt-Sigma pipeline directory (transformers
``T5EncoderModel``; ``pipe.encode_prompt`` at train_pixart_sigma.py:68-74,97-108), forward only, bf16.

The text side runs packed: ``encode`` takes the prompts' token ids as a list of 1-D tensors, lays them end to end as the rows
of one matrix and computes no pad row.  That is exact, not an approximation: the reference pads on the right, the pad keys are
masked for every real query, and the relative-position bias depends only on the distance key - query, so the real rows of a
padded batch equal the prompt encoded alone (a tiny fp32 transformers ``T5EncoderModel`` gives the 23 real rows of a
300-padded input bit-identical to the same ids alone; tests/test_t5_cpu.py holds the restatement to that).

Per block (T5Block of an encoder): ``layer.0.layer_norm`` (on the first block; afterwards fused with the residual add that
precedes it) -> q|k|v projection (one GEMM) -> attention with the relative-position bias -> ``o`` -> residual add +
``layer.1.layer_norm`` (one kernel) -> wi_0|wi_1 projection (one GEMM) -> gated GELU -> ``wo``; after the last block the final
residual add + ``final_layer_norm``.  Rounding points are those of the bf16 module except the gated GELU, which rounds the
activation once (include/yat_hip.h, "T5 v1.1 text encoder").

The relative-position bias exists in block 0 only and is shared by all blocks; ``relative_bias_table`` turns its
``[num_buckets, H]`` weight into the ``[H, 2 * max_len - 1]`` per-distance table the kernel looks up.  A prompt longer than
``MAX_PROMPT`` = 512 tokens is refused (PixArt-Sigma uses 300).
"""
from __future__ import annotations

import math

import torch

from .text_common import TextEncoderHIP, read_text_encoder_tensors
from .vae_common import BF16, check_expected, read_config

MAX_PROMPT = 512                      # yat_t5_attn_fwd's bound on one prompt

_REL = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
_EMBED = ("shared.weight", "encoder.embed_tokens.weight")


def validate_config(cfg: dict) -> None:
    """Refuse what the kernels do not compute."""
    ffp = cfg.get("feed_forward_proj", "relu")
    if ffp != "gated-gelu":
        raise NotImplementedError(f"T5 feed_forward_proj {ffp!r}: only gated-gelu (T5 v1.1) is built")
    if int(cfg.get("d_kv", 0)) != 64:
        raise NotImplementedError(f"T5 d_kv {cfg.get('d_kv')}: the attention kernel is built for 64")
    if cfg.get("is_decoder", False):
        raise NotImplementedError("T5 is_decoder = true: only the encoder stack is built")
    if cfg.get("is_encoder_decoder", False) and "T5EncoderModel" not in (cfg.get("architectures") or []):
        raise NotImplementedError("T5 is_encoder_decoder = true without the T5EncoderModel architecture: the directory holds "
                                  "no encoder-only stack")
    if int(cfg["d_model"]) % 8 or int(cfg["d_ff"]) % 8:
        raise NotImplementedError("d_model and d_ff must be multiples of 8")
    if int(cfg.get("relative_attention_num_buckets", 32)) % 2:
        raise ValueError("relative_attention_num_buckets must be even (bidirectional buckets)")


def expected_keys(cfg: dict) -> dict:
    """{key: shape} of a T5EncoderModel state dict, the tied embedding under ``shared.weight``."""
    D, F, H, dh = int(cfg["d_model"]), int(cfg["d_ff"]), int(cfg["num_heads"]), int(cfg["d_kv"])
    want = {"shared.weight": (int(cfg["vocab_size"]), D), "encoder.final_layer_norm.weight": (D,),
            _REL: (int(cfg.get("relative_attention_num_buckets", 32)), H)}
    for i in range(int(cfg["num_layers"])):
        p = f"encoder.block.{i}."
        for n in "qkv":
            want[p + f"layer.0.SelfAttention.{n}.weight"] = (H * dh, D)
        want[p + "layer.0.SelfAttention.o.weight"] = (D, H * dh)
        want[p + "layer.0.layer_norm.weight"] = (D,)
        want[p + "layer.1.DenseReluDense.wi_0.weight"] = (F, D)
        want[p + "layer.1.DenseReluDense.wi_1.weight"] = (F, D)
        want[p + "layer.1.DenseReluDense.wo.weight"] = (D, F)
        want[p + "layer.1.layer_norm.weight"] = (D,)
    return want


def load_text_encoder_dir(te_dir: str):
    """A transformers T5EncoderModel directory -> (config dict, {key: bf16 tensor}).  Reads ``model.safetensors`` or the shards
    of ``model.safetensors.index.json``.  The tied embedding may be stored as ``shared.weight``, as
    ``encoder.embed_tokens.weight`` or as both (then they must be equal); it comes back as ``shared.weight``.  Stored dtypes
    vary (transformers keeps ``wo`` in fp32 for some loads): everything is cast to bf16, as ``pipe.to(torch.bfloat16)`` does
    (train_pixart_sigma.py:52-54).  A missing or unexpected key raises and names it."""
    cfg = read_config(te_dir)
    validate_config(cfg)
    sd = read_text_encoder_tensors(te_dir)
    a, b = (sd.pop(k, None) for k in _EMBED)
    if a is not None and b is not None and not (a.shape == b.shape and torch.equal(a.float(), b.float())):
        raise ValueError("T5: shared.weight and encoder.embed_tokens.weight are tied but the checkpoint stores them unequal")
    if a is not None or b is not None:
        sd["shared.weight"] = a if a is not None else b
    check_expected(expected_keys(cfg), sd, lambda k: True, "T5", "T5EncoderHIP")
    return cfg, {k: v.to(BF16) for k, v in sd.items()}


def relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """``T5Attention._relative_position_bucket(bidirectional=True)``, op for op: fp32 log, ``.long()`` truncation, clamp."""
    num_buckets //= 2
    buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    if_large = max_exact + (torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact)
                            * (num_buckets - max_exact)).to(torch.long)
    if_large = torch.min(if_large, torch.full_like(if_large, num_buckets - 1))
    return buckets + torch.where(is_small, relative_position, if_large)


def relative_bias_table(weight, num_buckets, max_distance, max_len):
    """``relative_attention_bias.weight`` ``[num_buckets, H]`` -> bf16 ``[H, 2 * max_len - 1]``: column ``d + max_len - 1`` is
    the bias of relative position ``d`` = key index - query index, so ``compute_bias(L, L)[0, h, i, j]`` is
    ``table[h, (j - i) + max_len - 1]`` for every ``L <= max_len``."""
    rel = torch.arange(-(max_len - 1), max_len, dtype=torch.long, device=weight.device)
    bucket = relative_position_bucket(rel, int(num_buckets), int(max_distance))
    return torch.nn.functional.embedding(bucket, weight).t().to(BF16).contiguous()


class T5EncoderHIP(TextEncoderHIP):
    """Host side of the T5 encoder: packed weights on the device and the activation buffers of the largest call."""
    model_type = "t5"
    load_text_encoder_dir = staticmethod(load_text_encoder_dir)
    EMPTY_HINT = "T5's tokenizer always appends </s>"
    MAX_PROMPT_RULE = "min(512, n_positions)"

    def __init__(self, cfg: dict, sd: dict, device="cuda"):
        validate_config(cfg)
        super().__init__(cfg, device)
        self.d_model, self.d_ff, self.dh = int(cfg["d_model"]), int(cfg["d_ff"]), int(cfg["d_kv"])
        self.heads, self.L = int(cfg["num_heads"]), int(cfg["num_layers"])
        self.H = self.d_model                                      # the width of an embedding row, as Gemma2EncoderHIP.H
        self.eps = float(cfg.get("layer_norm_epsilon", 1e-6))
        self.num_buckets = int(cfg.get("relative_attention_num_buckets", 32))
        self.max_distance = int(cfg.get("relative_attention_max_distance", 128))
        self.max_prompt = min(MAX_PROMPT, int(cfg.get("n_positions") or MAX_PROMPT))
        dev = self.dev
        self.embed = dev(sd["shared.weight"] if "shared.weight" in sd else sd["encoder.embed_tokens.weight"])
        self.norm = dev(sd["encoder.final_layer_norm.weight"])
        self.rel_weight = dev(sd[_REL])
        self.layers = []
        for i in range(self.L):
            p = f"encoder.block.{i}."
            a, f = p + "layer.0.SelfAttention.", p + "layer.1.DenseReluDense."
            self.layers.append({
                "qkv": dev(torch.cat([sd[a + "q.weight"], sd[a + "k.weight"], sd[a + "v.weight"]], 0)),
                "o": dev(sd[a + "o.weight"]),
                "wi": dev(torch.cat([sd[f + "wi_0.weight"], sd[f + "wi_1.weight"]], 0)),
                "wo": dev(sd[f + "wo.weight"]),
                "ln0": dev(sd[p + "layer.0.layer_norm.weight"]),
                "ln1": dev(sd[p + "layer.1.layer_norm.weight"])})
        self._tables = {}

    def describe(self) -> str:
        return (f"T5 v1.1 text encoder on HIP: {self.L} blocks, d_model {self.d_model}, {self.heads} heads of {self.dh}, d_ff "
                f"{self.d_ff}; relative-position bias of {self.num_buckets} buckets up to distance {self.max_distance}, unscaled "
                "bidirectional attention, gated GELU rounded once")

    def free(self) -> None:
        super().free()
        self._tables = {}

    def _table(self, max_len: int):
        """The per-distance bias table of ``max_len`` rounded up to 64 (one entry kept per size)."""
        n = min((max_len + 63) // 64 * 64, MAX_PROMPT)
        if n not in self._tables:
            self._tables = {n: relative_bias_table(self.rel_weight, self.num_buckets, self.max_distance, n)}
        return n, self._tables[n]

    def _buffer_widths(self):
        return {"h": self.d_model, "n": self.d_model, "s": self.d_model, "qkv": 3 * self.heads * self.dh,
                "a": self.heads * self.dh, "wi": 2 * self.d_ff, "act": self.d_ff}

    def _forward(self, pack, bufs, y):
        from . import ops
        ids, off_d, rows, B = pack.ids, pack.off_d, pack.rows, len(pack.lens)
        max_len, table = self._table(max(pack.lens))
        h, n, s, qkv, a, wi, act = (bufs[k] for k in ("h", "n", "s", "qkv", "a", "wi", "act"))
        D, F, dh, H = self.d_model, self.d_ff, self.dh, self.heads
        ops.embed_rows(ids, self.embed, 1.0, h)
        for i, w in enumerate(self.layers):
            if i == 0:
                ops.t5_rmsnorm(h, w["ln0"], n, self.eps)
            else:
                ops.t5_rmsnorm(s, w["ln0"], n, self.eps, residual=h)          # h += the previous block's wo output
            ops.gemm(n, w["qkv"], qkv, M=rows, N=3 * H * dh, K=D)
            ops.t5_attn_fwd(qkv, off_d, B, H, dh, max_len, table, a)
            ops.gemm(a, w["o"], s, M=rows, N=D, K=H * dh)
            ops.t5_rmsnorm(s, w["ln1"], n, self.eps, residual=h)
            ops.gemm(n, w["wi"], wi, M=rows, N=2 * F, K=D)
            ops.geglu(wi, F, act)
            ops.gemm(act, w["wo"], s, M=rows, N=D, K=F)
        ops.t5_rmsnorm(s, self.norm, y, self.eps, residual=h)
