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

from yat_amd import dcae  # noqa: E402
from vae_bench_common import PEAK, conv_rows, instrumented, random_weights, timed  # noqa: E402

SANA_F32C32 = {"latent_channels": 32, "attention_head_dim": 32, "in_channels": 3,
               "decoder_block_out_channels": [128, 256, 512, 512, 1024, 1024],
               "decoder_block_types": ["ResBlock"] * 3 + ["EfficientViTBlock"] * 3, "decoder_layers_per_block": [3] * 6,
               "decoder_qkv_multiscales": [[], [], [], [5], [5], [5]], "decoder_norm_types": "rms_norm",
               "decoder_act_fns": "silu", "upsample_block_type": "interpolate", "scaling_factor": 0.41407}


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
    dec = dcae.AutoencoderDCDecoderHIP(cfg, dcae.pack_weights(cfg, random_weights(dcae.expected_keys(cfg))), device="cuda")
    lat = torch.randn(1, 32, a.latent, a.latent, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()
    for _ in range(a.warmup):
        dec.decode(lat)
    torch.cuda.synchronize()
    ms, times, img = timed(lambda: dec.decode(lat), a.repeats)
    flops = model_flops(cfg, a.latent, a.latent)

    # instrumented pass: an event pair around every 3x3 conv
    rec = instrumented({"dcae_conv3x3": lambda x, w, y, B, H, W, Cin, Cout, **kw: (
        (Cin, Cout, H, W, int(bool(kw.get("upsample")))), 2.0 * 9 * Cin * Cout * B * H * W)}, lambda: dec.decode(lat))
    conv_ms, per_shape = conv_rows(rec["dcae_conv3x3"], ("cin", "cout", "h", "w", "upsample"))
    print(json.dumps({"metric": "dcae_decode_ms", "image_px": 32 * a.latent, "ms_per_image": round(ms, 3),
                      "all_ms": [round(t, 3) for t in times], "model_tflop": round(flops / 1e12, 3),
                      "tflops": round(flops / ms / 1e9, 1), "frac_peak": round(flops / (ms * 1e-3) / PEAK, 3),
                      "conv3x3_ms_instrumented": round(conv_ms, 3), "conv3x3": per_shape,
                      "finite": bool(torch.isfinite(img.float()).all())}))


if __name__ == "__main__":
    main()
