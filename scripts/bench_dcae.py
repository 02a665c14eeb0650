#!/usr/bin/env python3
"""Side measurement (not a gate): one SANA DC-AE f32c32 decode of a 1024-px image (32 x 32 latent) on the HIP decoder,
random weights of the real widths.  Timed with HIP events after warm-up; prints one JSON line:

    ms per image, decoder TF/s (3x3 convs + 1x1 / Linear GEMMs counted), fraction of the 2.5 PF bf16 dense peak, and per
    3x3-conv shape (Cin, Cout, H, W, upsample): calls, ms, TF/s, fraction of peak (from an instrumented pass with an
    event pair around every conv launch).

    python scripts/bench_dcae.py [--latent 32] [--warmup 2] [--repeats 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yat_amd import dcae, ops  # noqa: E402

PEAK = 2.5e15
SANA_F32C32 = {"latent_channels": 32, "attention_head_dim": 32, "in_channels": 3,
               "decoder_block_out_channels": [128, 256, 512, 512, 1024, 1024],
               "decoder_block_types": ["ResBlock"] * 3 + ["EfficientViTBlock"] * 3, "decoder_layers_per_block": [3] * 6,
               "decoder_qkv_multiscales": [[], [], [], [5], [5], [5]], "decoder_norm_types": "rms_norm",
               "decoder_act_fns": "silu", "upsample_block_type": "interpolate", "scaling_factor": 0.41407}


def random_weights(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in dcae.expected_keys(cfg).items():
        if len(shape) == 1:
            sd[k] = (torch.ones(shape) if "norm" in k else 0.05 * torch.randn(shape, generator=g))
        else:
            fan = 1
            for s in shape[1:]:
                fan *= s
            sd[k] = torch.randn(shape, generator=g) / fan ** 0.5
    return sd


def model_flops(cfg, h, w):
    """Multiply-adds x 2 of the 3x3 convs and the GEMMs of one decode."""
    ch, n = cfg.block_out_channels, cfg.num_stages
    sizes = [(h << (n - 1 - i)) * (w << (n - 1 - i)) for i in range(n)]
    f = 2 * 9 * cfg.latent_channels * ch[-1] * sizes[-1] + 2 * 9 * ch[0] * cfg.out_channels * sizes[0]
    for i in range(n):
        c, px = ch[i], sizes[i]
        if i < n - 1:
            f += 2 * 9 * ch[i + 1] * c * px
        per = 2 * 2 * 9 * c * c * px if cfg.block_types[i] == dcae.RES else 2 * px * c * c * (3 + 2 + 8 + 4)
        f += cfg.layers_per_block[i] * per
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    cfg = dcae.parse_config(SANA_F32C32)
    dec = dcae.AutoencoderDCDecoderHIP(cfg, dcae.pack_weights(cfg, random_weights(cfg)), device="cuda")
    lat = torch.randn(1, 32, a.latent, a.latent, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()
    for _ in range(a.warmup):
        img = dec.decode(lat)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        img = dec.decode(lat)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = sorted(times)[len(times) // 2]
    flops = model_flops(cfg, a.latent, a.latent)

    # instrumented pass: an event pair around every 3x3 conv
    rec = []
    orig = ops.dcae_conv3x3

    def timed(x, w, y, B, H, W, Cin, Cout, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig(x, w, y, B, H, W, Cin, Cout, **kw)
        e1.record()
        rec.append(((Cin, Cout, H, W, int(bool(kw.get("upsample")))), 2.0 * 9 * Cin * Cout * B * H * W, e0, e1))
        return out
    ops.dcae_conv3x3 = timed
    try:
        dec.decode(lat)
        torch.cuda.synchronize()
    finally:
        ops.dcae_conv3x3 = orig
    shapes = {}
    for key, f, e0, e1 in rec:
        s = shapes.setdefault(key, [0, 0.0, 0.0])
        s[0] += 1
        s[1] += e0.elapsed_time(e1)
        s[2] += f
    conv_ms = sum(v[1] for v in shapes.values())
    per_shape = [{"cin": k[0], "cout": k[1], "h": k[2], "w": k[3], "upsample": k[4], "calls": v[0], "ms": round(v[1], 3),
                  "tflops": round(v[2] / v[1] / 1e9, 1), "frac_peak": round(v[2] / v[1] / 1e-3 / PEAK, 3)}
                 for k, v in sorted(shapes.items(), key=lambda kv: -kv[1][1])]
    print(json.dumps({"metric": "dcae_decode_ms", "image_px": 32 * a.latent, "ms_per_image": round(ms, 3),
                      "all_ms": [round(t, 3) for t in times], "model_tflop": round(flops / 1e12, 3),
                      "tflops": round(flops / ms / 1e9, 1), "frac_peak": round(flops / (ms * 1e-3) / PEAK, 3),
                      "conv3x3_ms_instrumented": round(conv_ms, 3), "conv3x3": per_shape,
                      "finite": bool(torch.isfinite(img.float()).all())}))


if __name__ == "__main__":
    main()
