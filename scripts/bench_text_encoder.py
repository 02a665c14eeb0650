#!/usr/bin/env python3
"""Side measurement (not a gate): a text encoder at its real shape on the HIP encoder with random bf16 weights made on the
device.  ``--kind gemma2``: SANA's, Gemma-2-2B's shape (26 layers, 2304 wide, 8 / 4 heads of 256, MLP 9216, vocabulary 256000);
``--kind t5``: PixArt-Sigma's, T5-XXL's encoder shape (24 blocks, d_model 4096, 64 heads of 64, d_ff 10240, vocabulary 32128);
``--kind clip``: SD3.5's two CLIP text encoders, one after the other in one line (``shapes``): CLIP-L's shape (12 blocks, 768
wide, 12 heads of 64, MLP 3072, quick-GELU) and OpenCLIP bigG's (32 blocks, 1280 wide, 20 heads of 64, MLP 5120, GELU), both
with the 49408-token vocabulary, at prompts of 77 tokens.
B = 1 and B = 8 prompts of 300 tokens (CLIP: 77), timed with HIP events after warm-up; prints one JSON line:

    per batch size: ms per call (median; every repeat listed), tokens per second, the share of each kernel kind in an
    instrumented pass (an event pair around every launch; attention's share is ``share.gemma_attn_fwd`` / ``share.t5_attn_fwd``),
    the GEMM and attention rates that pass reached, and both floors: the weight bytes at the HBM rate measured in this run (a
    device-to-device copy of 1 GiB, read + write counted) and the GEMM FLOPs at the project's measured 1120 TFLOP/s.

    python scripts/bench_text_encoder.py [--kind gemma2|t5|clip] [--layers N] [--tokens 300] [--batches 1 8] [--warmup 3] [--repeats 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yat_amd import clip, gemma2, t5  # noqa: E402
from vae_bench_common import instrumented, timed  # noqa: E402

BF = torch.bfloat16
GEMM_TFLOPS = 1120.0


def gemma2_2b(layers):
    return dict(hidden_size=2304, num_hidden_layers=layers, num_attention_heads=8, num_key_value_heads=4, head_dim=256,
                intermediate_size=9216, vocab_size=256000, rms_norm_eps=1e-6, query_pre_attn_scalar=256,
                attn_logit_softcapping=50.0, sliding_window=4096, max_position_embeddings=8192,
                hidden_activation="gelu_pytorch_tanh", attention_bias=False, rope_theta=10000.0)


def t5_xxl(layers):
    return dict(architectures=["T5EncoderModel"], model_type="t5", d_model=4096, num_layers=layers, num_heads=64, d_kv=64,
                d_ff=10240, vocab_size=32128, layer_norm_epsilon=1e-6, relative_attention_num_buckets=32,
                relative_attention_max_distance=128, feed_forward_proj="gated-gelu", is_encoder_decoder=False)


def clip_shape(hidden, heads, mlp, act, projection):
    def config(layers):
        return dict(architectures=["CLIPTextModelWithProjection"], model_type="clip_text_model", hidden_size=hidden,
                    num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=mlp, hidden_act=act,
                    projection_dim=projection, max_position_embeddings=77, vocab_size=49408, layer_norm_eps=1e-5, eos_token_id=2)
    return config


def clip_std(k, shape):
    """(mean, std) of one CLIP weight: norm weights around 1, biases small, matrices at the fan-in scale."""
    if len(shape) == 1:
        return (1.0, 0.1) if "layer_norm" in k and k.endswith(".weight") else (0.0, 0.1)
    return 0.0, 1.0 if "embedding" in k else shape[1] ** -0.5


def clip_kind(metric, layers, config):
    return dict(
        metric=metric, layers=layers, config=config, module=clip, cls=clip.CLIPTextEncoderHIP, std=clip_std, tokens=77,
        kinds=("gemm", "clip_attn_fwd", "clip_layernorm", "clip_act", "clip_embed"), attn="clip_attn_fwd",
        params=lambda e: 4 * e.hidden * e.hidden + 2 * e.ff * e.hidden,
        heads=lambda e: e.heads, pairs=lambda n: n * (n + 1) / 2, header=lambda e: {"hidden_act": e.act})


def gemma2_std(k, shape):
    """(mean, std) of one Gemma-2 weight: norm weights around 0 (the norm adds 1), matrices at the fan-in scale."""
    if len(shape) == 1:
        return 0.0, 0.1
    return 0.0, 1.0 if k == "embed_tokens.weight" else shape[1] ** -0.5


def t5_std(k, shape):
    """(mean, std) of one T5 weight.  q / k at 0.35 of the fan-in scale: T5 has no 1 / sqrt(dh), its trained projections
    carry that factor."""
    if len(shape) == 1:
        return 1.0, 0.1
    if "relative_attention_bias" in k or k == "shared.weight":
        return 0.0, 1.0
    return 0.0, shape[1] ** -0.5 * (0.35 if k.endswith((".q.weight", ".k.weight")) else 1.0)


# per kind: metric, default layers, config, module, encoder class, weight rule, kernel kinds, the attention kind,
# layer_params(encoder), attention (query, key) pairs of one prompt of n tokens (causal or full), extra header fields
KIND = {
    "gemma2": dict(
        metric="gemma2_encode_ms", layers=26, config=gemma2_2b, module=gemma2, cls=gemma2.Gemma2EncoderHIP, std=gemma2_std,
        kinds=("gemm", "gemma_attn_fwd", "gemma_rmsnorm", "rope_qk", "geglu", "embed_rows"), attn="gemma_attn_fwd",
        params=lambda e: (e.Hq + 2 * e.Hkv) * e.dh * e.H + e.H * e.Hq * e.dh + 2 * e.I * e.H + e.H * e.I,
        heads=lambda e: e.Hq, pairs=lambda n: n * (n + 1) / 2, header=lambda e: {"softcap": e.softcap}),
    "t5": dict(
        metric="t5_encode_ms", layers=24, config=t5_xxl, module=t5, cls=t5.T5EncoderHIP, std=t5_std,
        kinds=("gemm", "t5_attn_fwd", "t5_rmsnorm", "geglu", "embed_rows"), attn="t5_attn_fwd",
        params=lambda e: 4 * e.heads * e.dh * e.d_model + 3 * e.d_ff * e.d_model,
        heads=lambda e: e.heads, pairs=lambda n: n * n, header=lambda e: {}),
    "clip_l": clip_kind("clip_l_encode_ms", 12, clip_shape(768, 12, 3072, "quick_gelu", 768)),
    "clip_g": clip_kind("clip_g_encode_ms", 32, clip_shape(1280, 20, 5120, "gelu", 1280)),
}
GROUPS = {"clip": ("clip_l", "clip_g")}                       # a --kind that runs several shapes into one line


def device_weights(kind, cfg, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for k, shape in kind["module"].expected_keys(cfg).items():
        mean, std = kind["std"](k, shape)
        if len(shape) == 1:
            sd[k] = (mean + std * torch.randn(shape, generator=g, device="cuda")).to(BF)
        else:
            sd[k] = torch.randn(shape, generator=g, device="cuda", dtype=BF) * std
    return sd


def hbm_rate(repeats=10):
    """Bytes per second of a 1 GiB device-to-device copy (read + write)."""
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda").zero_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    ms, _, _ = timed(lambda: dst.copy_(src), repeats)
    return 2.0 * src.numel() / (ms * 1e-3)


def flat(res):
    """The tensors of an encode() result: rows per prompt, or CLIP's (rows, pooled) pairs."""
    return [t for r in res for t in (r if isinstance(r, (tuple, list)) else (r,))]


def measure(kind, a, rate):
    layers = a.layers or kind["layers"]
    tokens = a.tokens or kind.get("tokens", 300)
    a = argparse.Namespace(**{**vars(a), "tokens": tokens})
    cfg = kind["config"](layers)
    enc = kind["cls"](cfg, device_weights(kind, cfg), device="cuda")
    layer_params = kind["params"](enc)
    weight_bytes = 2.0 * layer_params * layers
    out = {"metric": kind["metric"], "layers": layers, "tokens_per_prompt": a.tokens, **kind["header"](enc),
           "hbm_bytes_per_s_measured": round(rate / 1e9, 1) * 1e9, "weight_gb": round(weight_bytes / 1e9, 3),
           "gemm_tflops_assumed": GEMM_TFLOPS, "batches": []}
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        prompts = [torch.randint(1, cfg["vocab_size"], (a.tokens,), generator=g) for _ in range(B)]
        for _ in range(a.warmup):
            enc.encode(prompts)
        torch.cuda.synchronize()
        ms, times, res = timed(lambda: enc.encode(prompts), a.repeats)
        rows = B * a.tokens
        # attention: two products of dh multiply-adds per (query, key, head)
        attn_flops = 2.0 * 2 * enc.dh * kind["heads"](enc) * B * kind["pairs"](a.tokens) * layers
        gemm_flops = 2.0 * rows * layer_params * layers
        rec = instrumented({k: (lambda *x, _k=k, **kw: (_k, 0.0)) for k in kind["kinds"]}, lambda: enc.encode(prompts))
        kind_ms = {k: sum(t for _, _, t in r) for k, r in rec.items()}
        total = sum(kind_ms.values())
        floor_w, floor_f = weight_bytes / rate * 1e3, gemm_flops / (GEMM_TFLOPS * 1e12) * 1e3
        out["batches"].append({
            "prompts": B, "rows": rows, "ms_per_call": round(ms, 3), "all_ms": [round(t, 3) for t in times],
            "tokens_per_s": round(rows / (ms * 1e-3)), "gemm_tflop": round(gemm_flops / 1e12, 3),
            "attn_tflop": round(attn_flops / 1e12, 4), "floor_ms_weights_at_hbm_rate": round(floor_w, 3),
            "floor_ms_gemm_flops": round(floor_f, 3), "ms_over_larger_floor": round(ms / max(floor_w, floor_f), 2),
            "instrumented_ms": {k: round(v, 3) for k, v in kind_ms.items()},
            "share": {k: round(v / total, 3) for k, v in kind_ms.items()},
            "gemm_tflops_reached": round(gemm_flops / 1e9 / max(kind_ms["gemm"], 1e-9), 1),
            "attn_tflops_reached": round(attn_flops / 1e9 / max(kind_ms[kind["attn"]], 1e-9), 1),
            "finite": bool(all(torch.isfinite(r.float()).all() for r in flat(res)))})
    enc.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=sorted(set(KIND) - {k for g in GROUPS.values() for k in g} | set(GROUPS)), default="gemma2")
    ap.add_argument("--layers", type=int, help="default: the model's own (26 / 24; CLIP: 12 and 32)")
    ap.add_argument("--tokens", type=int, help="default: 300 (CLIP: 77)")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    rate = hbm_rate()
    if a.kind in GROUPS:
        print(json.dumps({"metric": a.kind + "_encode_ms", "shapes": [measure(KIND[k], a, rate) for k in GROUPS[a.kind]]}))
    else:
        print(json.dumps(measure(KIND[a.kind], a, rate)))


if __name__ == "__main__":
    main()
