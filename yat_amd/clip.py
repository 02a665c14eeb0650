"""CLIP text encoder on the HIP kernels: ``text_encoder`` (CLIP-L) and ``text_encoder_2`` (OpenCLIP bigG) of an SD3.5 pipeline
directory (transformers ``CLIPTextModelWithProjection``; ``pipe.encode_prompt`` at train_sd35.py:79-92,113-118), forward only,
bf16.

``encode`` takes the prompts' token ids as a list of 1-D tensors, lays them end to end as the rows of one matrix and returns,
per prompt, the pair ``StableDiffusion3Pipeline._get_clip_prompt_embeds`` takes: ``hidden_states[-2]`` (the residual stream
entering the last block, no final norm) as ``[L, hidden]`` and ``text_embeds`` (``final_layer_norm`` of the last state's row at
the EOS position times ``text_projection``^T) as ``[projection_dim]``.  The model is causal, so a prompt's row depends on the
earlier rows only and encoding a prefix gives the prefix's rows exactly; the SD3 prompt rules (yat_amd/encode_prompts.py)
still feed all 77 ids, because the pad rows are part of ``prompt_embeds``.  Any length up to ``max_position_embeddings`` (at
most 512) is taken.

Per block (CLIPEncoderLayer): ``layer_norm1`` (on the first block; afterwards fused with the residual add that precedes it) ->
q|k|v projection (one GEMM with the concatenated bias) -> causal attention at ``scale = dh^-0.5`` -> ``out_proj`` + bias ->
residual add + ``layer_norm2`` (one kernel) -> ``fc1`` + bias -> quick-GELU or erf-GELU -> ``fc2`` + bias.  The fused
residual + norm that opens the last block stores exactly ``hidden_states[-2]``; it is directed to the output.  After the last
block only the B EOS rows take the final residual add, ``final_layer_norm`` and the projection.  Rounding points are those of
the bf16 module (include/yat_hip.h, "CLIP text encoder").

The EOS position is transformers' rule (modeling_clip.py): ``ids.argmax()`` when ``config.eos_token_id == 2`` (the configs
from before the id was corrected: CLIP's ``<|endoftext|>`` is the largest id of its vocabulary), else the first position whose
id is ``eos_token_id``.
"""
from __future__ import annotations

import torch

from .text_common import TextEncoderHIP, read_text_encoder_tensors
from .vae_common import BF16, check_expected, read_config

MAX_PROMPT = 512                      # yat_clip_attn_fwd's bound on one prompt
ACTS = ("quick_gelu", "gelu")


def validate_config(cfg: dict) -> None:
    """Refuse what the kernels do not compute."""
    D, H = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    if D % H or D // H != 64:
        raise NotImplementedError(f"CLIP head dim {D}/{H}: the attention kernel is built for 64")
    act = cfg.get("hidden_act", "quick_gelu")
    if act not in ACTS:
        raise NotImplementedError(f"CLIP hidden_act {act!r}: only quick_gelu (CLIP-L) and gelu (OpenCLIP bigG) are built")
    if int(cfg.get("max_position_embeddings", 77)) > MAX_PROMPT:
        raise NotImplementedError(f"CLIP max_position_embeddings {cfg['max_position_embeddings']}: the attention kernel is "
                                  f"built for at most {MAX_PROMPT}")
    if D % 8 or int(cfg["intermediate_size"]) % 8 or int(cfg.get("projection_dim", 512)) % 8:
        raise NotImplementedError("hidden_size, intermediate_size and projection_dim must be multiples of 8")


def expected_keys(cfg: dict) -> dict:
    """{key: shape} of a CLIPTextModelWithProjection state dict."""
    D, F = int(cfg["hidden_size"]), int(cfg["intermediate_size"])
    e = "text_model.embeddings."
    want = {e + "token_embedding.weight": (int(cfg["vocab_size"]), D),
            e + "position_embedding.weight": (int(cfg.get("max_position_embeddings", 77)), D),
            "text_model.final_layer_norm.weight": (D,), "text_model.final_layer_norm.bias": (D,),
            "text_projection.weight": (int(cfg.get("projection_dim", 512)), D)}
    for i in range(int(cfg["num_hidden_layers"])):
        p = f"text_model.encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            want[p + f"self_attn.{n}.weight"], want[p + f"self_attn.{n}.bias"] = (D, D), (D,)
        for n in ("layer_norm1", "layer_norm2"):
            want[p + n + ".weight"], want[p + n + ".bias"] = (D,), (D,)
        want[p + "mlp.fc1.weight"], want[p + "mlp.fc1.bias"] = (F, D), (F,)
        want[p + "mlp.fc2.weight"], want[p + "mlp.fc2.bias"] = (D, F), (D,)
    return want


def load_text_encoder_dir(te_dir: str):
    """A transformers CLIPTextModelWithProjection directory -> (config dict, {key: bf16 tensor}).  Reads ``model.safetensors`` or
    the shards of ``model.safetensors.index.json``.  A stored ``text_model.embeddings.position_ids`` (a buffer older
    transformers saved) is dropped unread; everything else is cast to bf16, as ``pipe.to(torch.bfloat16)`` does.  A missing or
    unexpected key raises and names it."""
    cfg = read_config(te_dir)
    validate_config(cfg)
    sd = read_text_encoder_tensors(te_dir, lambda k: None if k == "text_model.embeddings.position_ids" else k)
    check_expected(expected_keys(cfg), sd, lambda k: True, "CLIP", "CLIPTextEncoderHIP")
    return cfg, {k: v.to(BF16) for k, v in sd.items()}


def eos_position(ids: torch.Tensor, eos_token_id: int) -> int:
    """The row ``CLIPTextTransformer`` pools: ``ids.argmax()`` when ``eos_token_id == 2``, else the first ``eos_token_id``
    (position 0 when there is none, as the reference's ``argmax`` of an all-false comparison)."""
    if int(eos_token_id) == 2:
        return int(ids.to(torch.int32).argmax())
    return int((ids == int(eos_token_id)).to(torch.int32).argmax())


class CLIPTextEncoderHIP(TextEncoderHIP):
    """Host side of one CLIP text encoder: packed weights on the device and the activation buffers of the largest call."""
    model_type = "clip_text_model"
    load_text_encoder_dir = staticmethod(load_text_encoder_dir)
    EMPTY_HINT = "CLIP's tokenizer always writes <|startoftext|> and <|endoftext|>"
    MAX_PROMPT_RULE = "min(512, max_position_embeddings)"

    def __init__(self, cfg: dict, sd: dict, device="cuda"):
        validate_config(cfg)
        super().__init__(cfg, device)
        self.hidden, self.ff, self.heads = int(cfg["hidden_size"]), int(cfg["intermediate_size"]), int(cfg["num_attention_heads"])
        self.dh, self.L = self.hidden // self.heads, int(cfg["num_hidden_layers"])
        self.H = self.hidden                                       # the width of an embedding row, as T5EncoderHIP.H
        self.projection_dim = int(cfg.get("projection_dim", 512))
        self.eps = float(cfg.get("layer_norm_eps", 1e-5))
        self.act = cfg.get("hidden_act", "quick_gelu")
        self.eos_token_id = int(cfg.get("eos_token_id", 2))
        self.max_prompt = min(MAX_PROMPT, int(cfg.get("max_position_embeddings", 77)))
        dev = self.dev
        self.embed = dev(sd["text_model.embeddings.token_embedding.weight"])
        self.pos_embed = dev(sd["text_model.embeddings.position_embedding.weight"])
        self.norm_w, self.norm_b = dev(sd["text_model.final_layer_norm.weight"]), dev(sd["text_model.final_layer_norm.bias"])
        self.projection = dev(sd["text_projection.weight"])
        self.layers = []
        for i in range(self.L):
            p = f"text_model.encoder.layers.{i}."
            a = p + "self_attn."
            self.layers.append({
                "qkv": dev(torch.cat([sd[a + f"{n}_proj.weight"] for n in "qkv"], 0)),
                "qkv_b": dev(torch.cat([sd[a + f"{n}_proj.bias"] for n in "qkv"], 0)),
                "o": dev(sd[a + "out_proj.weight"]), "o_b": dev(sd[a + "out_proj.bias"]),
                "fc1": dev(sd[p + "mlp.fc1.weight"]), "fc1_b": dev(sd[p + "mlp.fc1.bias"]),
                "fc2": dev(sd[p + "mlp.fc2.weight"]), "fc2_b": dev(sd[p + "mlp.fc2.bias"]),
                "ln1": dev(sd[p + "layer_norm1.weight"]), "ln1_b": dev(sd[p + "layer_norm1.bias"]),
                "ln2": dev(sd[p + "layer_norm2.weight"]), "ln2_b": dev(sd[p + "layer_norm2.bias"])})
        self._eos_rows = self._pooled = None

    def describe(self) -> str:
        rule = "ids.argmax()" if self.eos_token_id == 2 else f"the first id {self.eos_token_id}"
        return (f"CLIP text encoder on HIP: {self.L} blocks, hidden {self.hidden}, {self.heads} heads of {self.dh}, MLP {self.ff} "
                f"with {self.act}, projection {self.projection_dim}; causal attention, hidden_states[-2] and text_embeds pooled at "
                f"{rule}")

    def _buffer_widths(self):
        return {"h": self.hidden, "n": self.hidden, "s": self.hidden, "qkv": 3 * self.hidden, "a": self.hidden, "f": self.ff}

    def _encode_chunk(self, prompts):
        """-> per prompt (``hidden_states[-2]`` [L, hidden], ``text_embeds`` [projection_dim])."""
        row0, rows = 0, []
        for p in prompts:
            rows.append(row0 + eos_position(p, self.eos_token_id))
            row0 += p.numel()
        self._eos_rows = torch.tensor(rows, dtype=torch.int64).to(self.device)
        hidden = super()._encode_chunk(prompts)
        pooled, self._pooled = self._pooled, None
        return [(h, pooled[b]) for b, h in enumerate(hidden)]

    def _forward(self, pack, bufs, y):
        from . import ops
        ids, off_d, rows, B = pack.ids, pack.off_d, pack.rows, len(pack.lens)
        pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in pack.lens]).to(self.device)
        max_len = max(pack.lens)
        h, n, s, qkv, a, f = (bufs[k] for k in ("h", "n", "s", "qkv", "a", "f"))
        D, F, dh, H, last = self.hidden, self.ff, self.dh, self.heads, self.L - 1
        scale = float(dh) ** -0.5
        ops.clip_embed(ids, pos, self.embed, self.pos_embed, y if last == 0 else h)
        for i, w in enumerate(self.layers):
            x = y if i == last else h                                 # the residual stream entering block i: y is hidden_states[-2]
            if i == 0:
                ops.clip_layernorm(x, w["ln1"], w["ln1_b"], n, self.eps)
            else:                                                      # h += the previous block's fc2 output
                ops.clip_layernorm(s, w["ln1"], w["ln1_b"], n, self.eps, residual=h, sum_out=x)
            ops.gemm(n, w["qkv"], qkv, M=rows, N=3 * D, K=D, bias=w["qkv_b"])
            ops.clip_attn_fwd(qkv, off_d, B, H, dh, max_len, scale, a)
            ops.gemm(a, w["o"], s, M=rows, N=D, K=D, bias=w["o_b"])
            ops.clip_layernorm(s, w["ln2"], w["ln2_b"], n, self.eps, residual=x, sum_out=h)   # (the last block leaves y alone)
            ops.gemm(n, w["fc1"], f, M=rows, N=F, K=D, bias=w["fc1_b"])
            ops.clip_act(f, self.act)
            ops.gemm(f, w["fc2"], s, M=rows, N=D, K=F, bias=w["fc2_b"])
        # the last state = h + s; only the B EOS rows take the final norm and the projection
        he, se = h.index_select(0, self._eos_rows), s.index_select(0, self._eos_rows)
        ne = torch.empty_like(he)
        ops.clip_layernorm(se, self.norm_w, self.norm_b, ne, self.eps, residual=he)
        self._pooled = torch.empty(B, self.projection_dim, dtype=BF16, device=self.device)
        ops.gemm(ne, self.projection, self._pooled, M=B, N=self.projection_dim, K=D)
