#!/usr/bin/env python3
"""Side measurement (not a gate): one AutoencoderKL decode of a 1024-px image (128 x 128 latent) on the HIP decoder at the
SDXL / PixArt-Sigma widths (4-channel latent, post_quant_conv) and at the SD3.5 widths (16-channel latent), random weights.
Timed with HIP events after warm-up; prints one JSON line with, per VAE:

    ms per image, decoder TF/s (3x3 convs + 1x1 / Linear GEMMs + attention counted), fraction of the 2.5 PF bf16 dense peak;
    from an instrumented pass with an event pair around every launch of a kind: per 3x3-conv shape (Cin, Cout, H, W,
    upsample) calls, ms, TF/s; GroupNorm ms and achieved GB/s (two reads and one write of its activation); attention ms and
    TF/s.

    python scripts/bench_vae_kl.py [--latent 128] [--warmup 2] [--repeats 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yat_amd import autoencoder_kl as kl  # noqa: E402
from vae_bench_common import PEAK, conv_rows, instrumented, random_weights, timed  # noqa: E402

WIDTHS = {"block_out_channels": [128, 256, 512, 512], "layers_per_block": 2, "norm_num_groups": 32, "act_fn": "silu",
          "up_block_types": ["UpDecoderBlock2D"] * 4, "mid_block_add_attention": True, "out_channels": 3}
VAES = {"sdxl": dict(WIDTHS, latent_channels=4, use_post_quant_conv=True, scaling_factor=0.13025),
        "sd35": dict(WIDTHS, latent_channels=16, use_post_quant_conv=False, scaling_factor=1.5305, shift_factor=0.0609)}


def model_flops(cfg, h, w):
    """Multiply-adds x 2 of the 3x3 convs, the GEMMs and the attention of one decode."""
    ch, L = cfg.block_out_channels, cfg.latent_channels
    mid, px = ch[-1], h * w
    f = 2 * L * L * px * cfg.use_post_quant_conv + 2 * 9 * L * mid * px
    res = [(px, mid, mid)] * 2
    rev = list(reversed(ch))
    prev, hh, ww = rev[0], h, w
    for i, c in enumerate(rev):
        res += [(hh * ww, prev if j == 0 else c, c) for j in range(cfg.layers_per_block + 1)]
        prev = c
        if i < len(rev) - 1:
            hh, ww = 2 * hh, 2 * ww
            f += 2 * 9 * c * c * hh * ww
    for n, cin, cout in res:
        f += 2 * 9 * n * (cin * cout + cout * cout) + (2 * n * cin * cout if cin != cout else 0)
    if cfg.mid_block_add_attention:
        f += 2 * px * mid * 4 * mid + 4 * px * px * mid
    return f + 2 * 9 * ch[0] * cfg.out_channels * hh * ww


def _instrument(dec, lat):
    """One decode with an event pair around every 3x3 conv, GroupNorm and attention launch."""
    rec = instrumented({
        "dcae_conv3x3": lambda x, w, y, B, H, W, Cin, Cout, **kw: (
            (Cin, Cout, H, W, int(bool(kw.get("upsample")))), 2.0 * 9 * Cin * Cout * B * H * W),
        "vae_groupnorm": lambda x, w, b, y, B, HW, C, *r, **kw: (None, 3.0 * 2 * B * HW * C),
        "vae_attn_fwd": lambda q, k, v, o, B, N, dh, *r, **kw: (None, 4.0 * B * N * N * dh)}, lambda: dec.decode(lat))
    conv_ms, per_shape = conv_rows(rec["dcae_conv3x3"], ("cin", "cout", "h", "w", "upsample"))
    gn, attn = rec["vae_groupnorm"], rec["vae_attn_fwd"]
    gn_ms, gn_bytes = sum(ms for _, _, ms in gn), sum(b for _, b, _ in gn)
    at_ms, at_f = sum(ms for _, _, ms in attn), sum(f for _, f, _ in attn)
    return {"conv3x3_ms_instrumented": round(conv_ms, 3), "conv3x3": per_shape,
            "groupnorm": {"calls": len(gn), "ms": round(gn_ms, 3), "gbytes": round(gn_bytes / 1e9, 2),
                          "gb_per_s": round(gn_bytes / gn_ms / 1e6, 1)},
            "attention": {"calls": len(attn), "ms": round(at_ms, 3), "tflop": round(at_f / 1e12, 3),
                          "tflops": round(at_f / at_ms / 1e9, 1) if at_ms else 0.0}}


def bench(raw, latent, warmup, repeats):
    cfg = kl.parse_config(raw)
    dec = kl.AutoencoderKLDecoderHIP(cfg, kl.pack_weights(cfg, random_weights(kl.expected_keys(cfg))), device="cuda")
    lat = torch.randn(1, cfg.latent_channels, latent, latent, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()
    for _ in range(warmup):
        dec.decode(lat)
    torch.cuda.synchronize()
    ms, times, img = timed(lambda: dec.decode(lat), repeats)
    flops = model_flops(cfg, latent, latent)
    out = {"image_px": 8 * latent, "ms_per_image": round(ms, 3), "all_ms": [round(t, 3) for t in times],
           "model_tflop": round(flops / 1e12, 3), "tflops": round(flops / ms / 1e9, 1),
           "frac_peak": round(flops / (ms * 1e-3) / PEAK, 3), "finite": bool(torch.isfinite(img.float()).all())}
    out.update(_instrument(dec, lat))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--vae", choices=sorted(VAES), action="append", help="default: both")
    a = ap.parse_args()
    res = {name: bench(VAES[name], a.latent, a.warmup, a.repeats) for name in (a.vae or sorted(VAES))}
    print(json.dumps({"metric": "vae_kl_decode_ms", **res}))


if __name__ == "__main__":
    main()
