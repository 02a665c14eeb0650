#!/usr/bin/env python3
"""Side measurement (not a gate): SANA's text encoder, Gemma-2-2B's shape (26 layers, 2304 wide, 8 / 4 heads of 256, MLP 9216,
vocabulary 256000), on the HIP encoder with random bf16 weights made on the device.  B = 1 and B = 8 prompts of 300 tokens,
timed with HIP events after warm-up; prints one JSON line:

    per batch size: ms per call (median; every repeat listed), tokens per second, the share of each kernel kind in an
    instrumented pass (an event pair around every launch; attention's share is ``share.gemma_attn_fwd``), and both floors:
    the per-layer weight bytes at the HBM rate measured in this run (a device-to-device copy of 1 GiB, read + write counted)
    and the GEMM FLOPs at the project's measured 1120 TFLOP/s.

    python scripts/bench_text_encoder.py [--layers 26] [--tokens 300] [--batches 1 8] [--warmup 3] [--repeats 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yat_amd import gemma2  # noqa: E402
from vae_bench_common import instrumented, timed  # noqa: E402

BF = torch.bfloat16
GEMM_TFLOPS = 1120.0
KINDS = ("gemm", "gemma_attn_fwd", "gemma_rmsnorm", "rope_qk", "geglu", "embed_rows")


def gemma2_2b(layers):
    return dict(hidden_size=2304, num_hidden_layers=layers, num_attention_heads=8, num_key_value_heads=4, head_dim=256,
                intermediate_size=9216, vocab_size=256000, rms_norm_eps=1e-6, query_pre_attn_scalar=256,
                attn_logit_softcapping=50.0, sliding_window=4096, max_position_embeddings=8192,
                hidden_activation="gelu_pytorch_tanh", attention_bias=False, rope_theta=10000.0)


def device_weights(cfg, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for k, shape in gemma2.expected_keys(cfg).items():
        if len(shape) == 1:
            sd[k] = (0.1 * torch.randn(shape, generator=g, device="cuda")).to(BF)
        else:
            std = 1.0 if k == "embed_tokens.weight" else shape[1] ** -0.5
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=26)
    ap.add_argument("--tokens", type=int, default=300)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    cfg = gemma2_2b(a.layers)
    enc = gemma2.Gemma2EncoderHIP(cfg, device_weights(cfg), device="cuda")
    H, I, dh, Hq, Hkv = enc.H, enc.I, enc.dh, enc.Hq, enc.Hkv
    layer_params = (Hq + 2 * Hkv) * dh * H + H * Hq * dh + 2 * I * H + H * I
    weight_bytes = 2.0 * layer_params * a.layers
    rate = hbm_rate()
    out = {"metric": "gemma2_encode_ms", "layers": a.layers, "tokens_per_prompt": a.tokens, "softcap": enc.softcap,
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
        # causal attention: rows of i + 1 keys, two products of dh multiply-adds per (query, key, head)
        attn_flops = 2.0 * 2 * dh * Hq * B * (a.tokens * (a.tokens + 1) / 2) * a.layers
        gemm_flops = 2.0 * rows * layer_params * a.layers
        rec = instrumented({k: (lambda *x, _k=k, **kw: (_k, 0.0)) for k in KINDS}, lambda: enc.encode(prompts))
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
            "finite": bool(all(torch.isfinite(r.float()).all() for r in res))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
