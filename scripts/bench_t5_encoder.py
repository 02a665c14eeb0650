#!/usr/bin/env python3
"""Side measurement (not a gate): PixArt-Sigma's text encoder, T5-XXL's encoder shape (24 blocks, d_model 4096, 64 heads of 64,
d_ff 10240, vocabulary 32128), on the HIP encoder with random bf16 weights made on the device.  B = 1 and B = 8 prompts of 300
tokens, timed with HIP events after warm-up; prints one JSON line:

    per batch size: ms per call (median; every repeat listed), tokens per second, the share of each kernel kind in an
    instrumented pass (an event pair around every launch; attention's share is ``share.t5_attn_fwd``), the GEMM rate that pass
    reached, and both floors: the weight bytes at the HBM rate measured in this run (a device-to-device copy of 1 GiB, read +
    write counted) and the GEMM FLOPs at the project's measured 1120 TFLOP/s for its GEMM family.

    python scripts/bench_t5_encoder.py [--layers 24] [--tokens 300] [--batches 1 8] [--warmup 3] [--repeats 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yat_amd import t5  # noqa: E402
from vae_bench_common import instrumented, timed  # noqa: E402

BF = torch.bfloat16
GEMM_TFLOPS = 1120.0
KINDS = ("gemm", "t5_attn_fwd", "t5_rmsnorm", "geglu", "embed_rows")


def t5_xxl(layers):
    return dict(architectures=["T5EncoderModel"], model_type="t5", d_model=4096, num_layers=layers, num_heads=64, d_kv=64,
                d_ff=10240, vocab_size=32128, layer_norm_epsilon=1e-6, relative_attention_num_buckets=32,
                relative_attention_max_distance=128, feed_forward_proj="gated-gelu", is_encoder_decoder=False)


def device_weights(cfg, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for k, shape in t5.expected_keys(cfg).items():
        if len(shape) == 1:
            sd[k] = (1.0 + 0.1 * torch.randn(shape, generator=g, device="cuda")).to(BF)
        elif "relative_attention_bias" in k or k == "shared.weight":
            sd[k] = torch.randn(shape, generator=g, device="cuda", dtype=BF)
        else:
            # q / k at 0.35 of the fan-in scale: T5 has no 1 / sqrt(dh), its trained projections carry that factor
            std = shape[1] ** -0.5 * (0.35 if k.endswith((".q.weight", ".k.weight")) else 1.0)
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
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--tokens", type=int, default=300)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    cfg = t5_xxl(a.layers)
    enc = t5.T5EncoderHIP(cfg, device_weights(cfg), device="cuda")
    D, F, dh, H = enc.d_model, enc.d_ff, enc.dh, enc.heads
    layer_params = 4 * H * dh * D + 3 * F * D
    weight_bytes = 2.0 * layer_params * a.layers
    rate = hbm_rate()
    out = {"metric": "t5_encode_ms", "layers": a.layers, "tokens_per_prompt": a.tokens,
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
        # bidirectional attention: every query sees every key, two products of dh multiply-adds per (query, key, head)
        attn_flops = 2.0 * 2 * dh * H * B * a.tokens * a.tokens * a.layers
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
            "gemm_tflops_reached": round(gemm_flops / 1e9 / max(kind_ms["gemm"], 1e-9), 1),
            "attn_tflops_reached": round(attn_flops / 1e9 / max(kind_ms["t5_attn_fwd"], 1e-9), 1),
            "finite": bool(all(torch.isfinite(r.float()).all() for r in res))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
