#!/usr/bin/env python3
"""Side measurement (not a gate): one AutoencoderKL encode of a 1024-px image on the HIP encoder at the SDXL / PixArt-Sigma
widths (4-channel latent, quant_conv) and at the SD3.5 widths (16-channel latent), random weights.  Timed with HIP events
after warm-up; prints one JSON line with, per VAE:

    ms per image (from bf16 and from uint8), encoder TF/s (3x3 convs + 1x1 / Linear GEMMs + attention counted), fraction of
    the 2.5 PF bf16 dense peak; from an instrumented pass with an event pair around every launch of a kind: per conv shape
    and kind (stride-1 conv3x3, Downsample2D) calls, ms, TF/s; GroupNorm ms and achieved GB/s (two reads and one write of
    its activation); attention and sampling-tail ms; and, with --torch-ref, the bf16 torch restatement of the tests on the
    same GPU, labelled as such;

and, once, every Downsample2D shape beside the stride-1 conv at the same (M, N, K), timed in the same run.

    python scripts/bench_vae_kl_encoder.py [--px 1024] [--warmup 2] [--repeats 5] [--torch-ref]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yat_amd import autoencoder_kl_encoder as ke, ops  # noqa: E402
from vae_bench_common import PEAK, conv_rows, instrumented, random_weights, timed  # noqa: E402

BF = torch.bfloat16
WIDTHS = {"block_out_channels": [128, 256, 512, 512], "layers_per_block": 2, "norm_num_groups": 32, "act_fn": "silu",
          "down_block_types": ["DownEncoderBlock2D"] * 4, "mid_block_add_attention": True, "in_channels": 3}
VAES = {"sdxl": dict(WIDTHS, latent_channels=4, use_quant_conv=True, scaling_factor=0.13025),
        "sd35": dict(WIDTHS, latent_channels=16, use_quant_conv=False, scaling_factor=1.5305, shift_factor=0.0609)}


def model_flops(cfg, H, W):
    """Multiply-adds x 2 of the 3x3 convs, the GEMMs and the attention of one encode (conv_in at its 3 real input channels)."""
    ch, m = cfg.block_out_channels, cfg.moment_channels
    f = 2 * 9 * cfg.in_channels * ch[0] * H * W
    prev, hh, ww = ch[0], H, W
    res = []
    for i, c in enumerate(ch):
        res += [(hh * ww, prev if j == 0 else c, c) for j in range(cfg.layers_per_block)]
        prev = c
        if i < len(ch) - 1:
            hh, ww = hh // 2, ww // 2
            f += 2 * 9 * c * c * hh * ww
    px, mid = hh * ww, ch[-1]
    res += [(px, mid, mid)] * 2
    for n, cin, cout in res:
        f += 2 * 9 * n * (cin * cout + cout * cout) + (2 * n * cin * cout if cin != cout else 0)
    if cfg.mid_block_add_attention:
        f += 2 * px * mid * 4 * mid + 4 * px * px * mid
    return f + 2 * 9 * mid * m * px + 2 * m * m * px * cfg.use_quant_conv


def _instrument(enc, img):
    """One encode with an event pair around every 3x3 conv, GroupNorm, attention and sampling launch."""
    def conv(name, stride):
        return lambda x, w, y, B, H, W, Cin, Cout, **kw: (
            (name, Cin, Cout, H, W), 2.0 * 9 * Cin * Cout * B * (H // stride) * (W // stride))
    rec = instrumented({
        "dcae_conv3x3": conv("dcae_conv3x3", 1), "vae_conv3x3_down": conv("vae_conv3x3_down", 2),
        "vae_groupnorm": lambda x, w, b, y, B, HW, C, *r, **kw: ((HW, C), 3.0 * 2 * B * HW * C),
        "vae_attn_fwd": lambda q, k, v, o, B, N, dh, *r, **kw: (None, 4.0 * B * N * N * dh),
        "vae_kl_sample": lambda *a, **kw: (None, 0.0)}, lambda: enc.encode(img))
    conv_ms, per_shape = conv_rows(rec["dcae_conv3x3"] + rec["vae_conv3x3_down"], ("kernel", "cin", "cout", "h_in", "w_in"))
    gn, attn = rec["vae_groupnorm"], rec["vae_attn_fwd"]
    gn_ms, gn_bytes = sum(ms for _, _, ms in gn), sum(b for _, b, _ in gn)
    top = max(gn, key=lambda r: r[2])
    return {"conv3x3_ms_instrumented": round(conv_ms, 3), "conv3x3": per_shape,
            "groupnorm": {"calls": len(gn), "ms": round(gn_ms, 3), "gbytes": round(gn_bytes / 1e9, 2),
                          "gb_per_s": round(gn_bytes / gn_ms / 1e6, 1),
                          "slowest": {"hw": top[0][0], "c": top[0][1], "ms": round(top[2], 3),
                                      "ms_all_of_that_shape": round(sum(ms for k, _, ms in gn if k == top[0]), 3)}},
            "attention_ms": round(sum(ms for _, _, ms in attn), 3),
            "kl_sample_ms": round(sum(ms for _, _, ms in rec["vae_kl_sample"]), 3)}


def bench(name, raw, px, warmup, repeats, torch_ref):
    cfg = ke.parse_encoder_config(raw)
    sd = random_weights(ke.expected_keys(cfg))
    enc = ke.AutoencoderKLEncoderHIP(cfg, ke.pack_weights(cfg, sd), device="cuda")
    img = (torch.rand(1, 3, px, px, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(BF).cuda()
    u8 = torch.randint(0, 256, (px, px, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).cuda()
    for _ in range(warmup):
        enc.encode(img)
        enc.encode_uint8(u8)
    torch.cuda.synchronize()
    ms, times, lat = timed(lambda: enc.encode(img), repeats)
    ms_u8, _, _ = timed(lambda: enc.encode_uint8(u8), repeats)
    flops = model_flops(cfg, px, px)
    out = {"image_px": px, "ms_per_image": round(ms, 3), "all_ms": [round(t, 3) for t in times],
           "ms_per_image_from_uint8": round(ms_u8, 3), "model_tflop": round(flops / 1e12, 3),
           "tflops": round(flops / ms / 1e9, 1), "frac_peak": round(flops / (ms * 1e-3) / PEAK, 3),
           "finite": bool(torch.isfinite(lat.float()).all())}
    out.update(_instrument(enc, img))
    if torch_ref:
        from tests import autoencoder_kl_encoder_ref as encref
        ref_cfg = {"latent_channels": cfg.latent_channels, "block_out_channels": list(cfg.block_out_channels),
                   "layers_per_block": cfg.layers_per_block, "norm_num_groups": cfg.norm_num_groups,
                   "scaling_factor": cfg.scaling_factor, "shift_factor": cfg.shift_factor,
                   "use_post_quant_conv": cfg.use_quant_conv, "mid_block_add_attention": cfg.mid_block_add_attention}
        sdb = {k: v.to(BF).cuda() for k, v in sd.items()}
        noise = torch.randn(1, cfg.latent_channels, px // 8, px // 8, device="cuda", dtype=BF)
        with torch.no_grad():
            encref.encode(ref_cfg, sdb, img, BF, noise)
            torch.cuda.synchronize()
            t, _, _ = timed(lambda: encref.encode(ref_cfg, sdb, img, BF, noise), repeats)
        out["torch_bf16_restatement_ms"] = round(t, 3)
    return out


def down_vs_stride1(px, repeats):
    """Every Downsample2D shape of the SD-family encoder against the stride-1 conv at the same (M, N, K)."""
    rows = []
    for i, c in enumerate(WIDTHS["block_out_channels"][:-1]):
        H = W = px >> i
        g = torch.Generator().manual_seed(i)
        x = torch.randn(H * W * c, generator=g).to(BF).cuda()
        w = (torch.randn(c, 3, 3, c, generator=g) / (9 * c) ** 0.5).to(BF).cuda()
        b = (0.05 * torch.randn(c, generator=g)).to(BF).cuda()
        y = torch.empty((H // 2) * (W // 2) * c, dtype=BF, device="cuda")
        f = 2.0 * 9 * c * c * (H // 2) * (W // 2)
        row = {"cin": c, "cout": c, "h_in": H, "m": (H // 2) * (W // 2), "n": c, "k": 9 * c}
        for label, fn in (("down", lambda: ops.vae_conv3x3_down(x, w, y, 1, H, W, c, c, bias=b)),
                          ("stride1", lambda: ops.dcae_conv3x3(x, w, y, 1, H // 2, W // 2, c, c, bias=b))):
            fn()
            torch.cuda.synchronize()
            t, _, _ = timed(fn, max(repeats, 5))
            row[label + "_ms"] = round(t, 4)
            row[label + "_frac_peak"] = round(f / (t * 1e-3) / PEAK, 3)
        row["stride1_over_down"] = round(row["stride1_ms"] / row["down_ms"], 3)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--px", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--vae", choices=sorted(VAES), action="append", help="default: both")
    ap.add_argument("--torch-ref", action="store_true", help="also time tests/autoencoder_kl_encoder_ref.py in bf16 on this GPU")
    a = ap.parse_args()
    res = {name: bench(name, VAES[name], a.px, a.warmup, a.repeats, a.torch_ref) for name in (a.vae or sorted(VAES))}
    print(json.dumps({"metric": "vae_kl_encode_ms", **res, "down_vs_stride1_same_mnk": down_vs_stride1(a.px, a.repeats)}))


if __name__ == "__main__":
    main()
