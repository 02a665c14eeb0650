#!/usr/bin/env python3
"""Side measurement (not a gate): one SANA DC-AE f32c32 encode of a 1024-px image on the HIP encoder, random weights of
the real widths.  Timed with HIP events after warm-up; prints one JSON line:

    ms per image, encoder TF/s (3x3 convs + 1x1 / Linear GEMMs counted), fraction of the 2.5 PF bf16 dense peak; per conv
    shape and kind (stride-1 conv3x3, stride-2 down, conv_out mean): calls, ms, TF/s, fraction of peak (from an instrumented
    pass with an event pair around every conv launch); for every down-block shape the stride-1 conv at the same (M, N, K)
    timed in the same run; and, with --torch-ref, the bf16 torch restatement of the tests on the same GPU, labelled as such.

    python scripts/bench_dcae_encoder.py [--px 1024] [--warmup 2] [--repeats 5] [--torch-ref]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yat_amd import dcae, dcae_encoder, ops  # noqa: E402
from vae_bench_common import PEAK, conv_rows, instrumented, random_weights, timed  # noqa: E402

BF = torch.bfloat16
SANA_F32C32 = {"latent_channels": 32, "attention_head_dim": 32, "in_channels": 3,
               "encoder_block_out_channels": [128, 256, 512, 512, 1024, 1024],
               "encoder_block_types": ["ResBlock"] * 3 + ["EfficientViTBlock"] * 3,
               "encoder_layers_per_block": [2, 2, 2, 3, 3, 3], "encoder_qkv_multiscales": [[], [], [], [5], [5], [5]],
               "downsample_block_type": "Conv", "scaling_factor": 0.41407}


def model_flops(cfg, H, W):
    """Multiply-adds x 2 of the 3x3 convs and the GEMMs of one encode (conv_in counted at its 3 real input channels)."""
    ch, n = cfg.block_out_channels, cfg.num_stages
    sizes = [(H >> i) * (W >> i) for i in range(n)]
    f = 2 * 9 * cfg.in_channels * ch[0] * sizes[0] + 2 * 9 * ch[-1] * cfg.latent_channels * sizes[-1]
    for i in range(n):
        c, px = ch[i], sizes[i]
        if i < n - 1:
            f += 2 * 9 * c * ch[i + 1] * sizes[i + 1]
        per = 2 * 2 * 9 * c * c * px if cfg.block_types[i] == dcae.RES else 2 * px * c * c * (3 + 2 + 8 + 4)
        f += cfg.layers_per_block[i] * per
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--px", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-ref", action="store_true", help="also time tests/dcae_encoder_ref.py in bf16 on this GPU")
    a = ap.parse_args()
    cfg = dcae_encoder.parse_encoder_config(SANA_F32C32)
    sd = random_weights(dcae_encoder.expected_keys(cfg))
    enc = dcae_encoder.AutoencoderDCEncoderHIP(cfg, dcae_encoder.pack_weights(cfg, sd), device="cuda")
    img = (torch.rand(1, 3, a.px, a.px, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(BF).cuda()
    u8 = torch.randint(0, 256, (a.px, a.px, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).cuda()
    for _ in range(a.warmup):
        enc.encode(img)
        enc.encode_uint8(u8)
    torch.cuda.synchronize()
    ms, times, lat = timed(lambda: enc.encode(img), a.repeats)
    ms_u8, _, _ = timed(lambda: enc.encode_uint8(u8), a.repeats)
    flops = model_flops(cfg, a.px, a.px)

    # instrumented pass: an event pair around every 3x3 conv of the three kinds
    def meter(name, stride):
        return lambda x, w, y, B, H, W, Cin, Cout, **kw: (
            (name, Cin, Cout, H, W), 2.0 * 9 * Cin * Cout * B * (H // stride) * (W // stride))
    rec = instrumented({n: meter(n, s) for n, s in (("dcae_conv3x3", 1), ("dcae_conv3x3_down", 2), ("dcae_conv3x3_mean", 1))},
                       lambda: enc.encode(img))
    conv_ms, per_shape = conv_rows(sum(rec.values(), []), ("kernel", "cin", "cout", "h_in", "w_in"))

    # every down-block shape against the stride-1 conv at the same (M, N, K): same output grid, same Cin and Cout
    ch = cfg.block_out_channels
    pairs = []
    for i in range(cfg.num_stages - 1):
        H = W = a.px >> i
        cin, cout = ch[i], ch[i + 1]
        x = torch.randn(H * W * cin, generator=torch.Generator().manual_seed(i)).to(BF).cuda()
        y = torch.empty((H // 2) * (W // 2) * cout, dtype=BF, device="cuda")
        w, b = enc.w[f"{i}.down.w"], enc.w[f"{i}.down.b"]
        f = 2.0 * 9 * cin * cout * (H // 2) * (W // 2)
        row = {"cin": cin, "cout": cout, "m": (H // 2) * (W // 2), "n": cout, "k": 9 * cin}
        for label, fn in (("down", lambda: ops.dcae_conv3x3_down(x, w, y, 1, H, W, cin, cout, bias=b)),
                          ("down_no_shortcut", lambda: ops.dcae_conv3x3_down(x, w, y, 1, H, W, cin, cout, bias=b, shortcut=False)),
                          ("stride1", lambda: ops.dcae_conv3x3(x, w, y, 1, H // 2, W // 2, cin, cout, bias=b))):
            fn()
            torch.cuda.synchronize()
            t, _, _ = timed(fn, max(a.repeats, 5))
            row[label + "_ms"] = round(t, 4)
            row[label + "_frac_peak"] = round(f / (t * 1e-3) / PEAK, 3)
        pairs.append(row)

    out = {"metric": "dcae_encode_ms", "image_px": a.px, "ms_per_image": round(ms, 3), "all_ms": [round(t, 3) for t in times],
           "ms_per_image_from_uint8": round(ms_u8, 3), "model_tflop": round(flops / 1e12, 3),
           "tflops": round(flops / ms / 1e9, 1), "frac_peak": round(flops / (ms * 1e-3) / PEAK, 3),
           "conv3x3_ms_instrumented": round(conv_ms, 3), "conv3x3": per_shape, "down_vs_stride1_same_mnk": pairs,
           "finite": bool(torch.isfinite(lat.float()).all())}
    if a.torch_ref:
        from tests import dcae_encoder_ref
        ref_cfg = {"latent_channels": 32, "block_out_channels": list(ch), "block_types": list(cfg.block_types),
                   "layers_per_block": list(cfg.layers_per_block), "scaling_factor": cfg.scaling_factor}
        sdb = {k: v.to(BF).cuda() for k, v in sd.items()}
        with torch.no_grad():
            dcae_encoder_ref.encode(ref_cfg, sdb, img, BF)
            torch.cuda.synchronize()
            t, _, _ = timed(lambda: dcae_encoder_ref.encode(ref_cfg, sdb, img, BF), a.repeats)
        out["torch_bf16_restatement_ms"] = round(t, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
