#!/usr/bin/env python3
"""SANA-1.5-1.6B 1024 px training step on one MI355X, side by side with the same model without the q/k norm -- a side
measurement, NOT the headline bench (that is bench.py, SANA-1.0-1.6B).  The workload is bench.py's: cached latents
[B, 32, h, w] over the 1024 px aspect buckets, prompt embeddings of 20..300 rows (packed text), flow matching, bf16 MSE,
clip 1.0 + AdamW; synthetic data, synthetic weights of the real architecture (20 blocks, D = 2240).

    python scripts/bench_sana15.py [--batch 8] [--steps 20] [--warmup 5] [--rounds 3] [--layers 20] [--only both|plain|qknorm]

Both models live in one process and are timed in alternating windows of ``--steps`` steps, ``--rounds`` windows each (same
box, same call, the spread between windows is printed).  ``--only qknorm`` runs the 1.5 model alone: the form to put behind a
kernel-trace profiler, in a run of its own.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

BUCKETS = [(32, 32), (16, 64), (24, 42), (44, 22)]            # bench.py's latent grids (h, w), all ~1024 tokens


def log(msg):
    print(f"[bench_sana15] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per model, alternating between the models")
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--only", choices=("both", "plain", "qknorm"), default="both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU (the HIP path has no CPU fallback)")
    from yat_amd.common.host import cap_host_threads
    cap_host_threads()
    dev = torch.device("cuda", 0)
    from yat_amd import ops
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    from yat_amd.recipe import SanaRecipe
    from yat_amd.optim import FlatAdamW

    B, T = args.batch, 512
    Cc = SanaConfig().caption_channels
    g = torch.Generator(device=dev).manual_seed(1234)
    hg = torch.Generator().manual_seed(1234)
    batches = []
    for (h, w) in BUCKETS:
        lat = (torch.randn(B, 32, h, w, generator=g, device=dev) * 0.5).to(torch.bfloat16)
        lens = torch.randint(20, 301, (B,), generator=hg).tolist()
        offs = [0]
        for L in lens:
            offs.append(offs[-1] + L)
        src = torch.randn(offs[-1], Cc, generator=g, device=dev).to(torch.bfloat16)
        batches.append(dict(lat=lat, src=src, offsets=torch.tensor(offs, dtype=torch.int32, device=dev),
                            work=ops.kv_work_list(lens, T, dev), lens=lens, rows=offs[-1]))

    def build(qk_norm):
        """one model with its optimizer, recipe and staging buffers; returns step(i)"""
        cfg = SanaConfig(num_layers=args.layers, qk_norm=qk_norm)
        model = SanaTransformer2DModelHIP(cfg, device=dev).init_synthetic(seed=0)
        opt = FlatAdamW(model, lr=1e-5, weight_decay=0.0, max_grad_norm=1.0, overlap_update=True)
        recipe = SanaRecipe(model, pad_to=T, device=dev)
        enc = torch.empty(B, T, Cc, dtype=torch.bfloat16, device=dev)
        mask = torch.empty(B, T, dtype=torch.int64, device=dev)
        bias = torch.empty(B, T, dtype=torch.float32, device=dev)
        kvl = torch.empty(B, dtype=torch.int32, device=dev)
        loss_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        t_dev = torch.empty(B, dtype=torch.float32, device=dev)
        sig_dev = torch.empty(B, dtype=torch.bfloat16, device=dev)
        noise_gen = torch.Generator(device=dev).manual_seed(99)
        ts_gen = torch.Generator().manual_seed(77)

        def step(i):
            b = batches[i % len(batches)]
            if recipe.packs_text(b["lens"]):
                enc_b, kv_off = recipe.packed_enc(B, T, Cc, b["rows"]), b["offsets"][:B]
                ops.pack_mask(b["src"], b["offsets"], B, T, Cc, enc_b, mask, bias, kvl)
            else:
                enc_b, kv_off = enc, None
                ops.pad_mask(b["src"], b["offsets"], B, T, Cc, enc, mask, bias, kvl)
            noise = torch.randn(b["lat"].shape, generator=noise_gen, device=dev, dtype=torch.bfloat16)
            _, t_host, sig_host = recipe.scheduler.sample(B, ts_gen)
            t_dev.copy_(t_host, non_blocking=True)
            sig_dev.copy_(sig_host, non_blocking=True)
            recipe.train_step_device(b["lat"], enc_b, (bias, kvl), noise, t_dev, sig_dev, loss_dev, kv_work=b["work"],
                                     kv_off=kv_off)
            opt.step()
        return SimpleRun(model, step, loss_dev)

    class SimpleRun:
        def __init__(self, model, step, loss_dev):
            self.model, self.step, self.loss_dev, self.ms, self.n = model, step, loss_dev, [], 0

        def window(self, steps, timed=True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                self.step(self.n)
                self.n += 1
            torch.cuda.synchronize()
            if timed:
                self.ms.append(1e3 * (time.perf_counter() - t0) / steps)

    tags = {"both": ("plain", "qknorm"), "plain": ("plain",), "qknorm": ("qknorm",)}[args.only]
    runs = {t: build(None if t == "plain" else "rms_norm_across_heads") for t in tags}
    for t, r in runs.items():
        log(f"{t}: {args.layers} blocks, {r.model.numel_flat / 1e6:.1f} M parameters; warm-up")
        r.window(args.warmup, timed=False)
        log(f"{t}: loss after warm-up {r.loss_dev.item():.4f}")
    for k in range(args.rounds):
        for t in (tags if k % 2 == 0 else tags[::-1]):              # alternate, and alternate who goes first
            runs[t].window(args.steps)
            log(f"round {k} {t}: {runs[t].ms[-1]:.2f} ms/step")
    res = {"metric": "ms/step SANA-1.5-1.6B (qk_norm = rms_norm_across_heads) 1024px bf16 training step beside the same model "
                     "without the q/k norm (side measurement)",
           "unit": "ms/step", "n_gpus": 1, "steps_per_window": args.steps, "windows": args.rounds, "warmup": args.warmup,
           "higher_is_better": False, "dtype": "bf16", "data": "synthetic",
           "config": {"per_gpu_batch": B, "layers": args.layers, "buckets": BUCKETS, "text": "20..300 rows per prompt, T = 512"},
           "hbm_peak_gb": torch.cuda.max_memory_allocated(dev) / 2 ** 30}
    for t, r in runs.items():
        res[t] = {"ms_per_step_windows": r.ms, "ms_per_step": statistics.median(r.ms), "images_per_s": 1e3 * B / statistics.median(r.ms),
                  "loss": r.loss_dev.item(), "params": r.model.numel_flat, "plan_replays": getattr(r.model, "plan_replays", 0)}
    if args.only == "both":
        res["value"] = res["qknorm"]["ms_per_step"]
        res["qknorm_minus_plain_ms"] = res["qknorm"]["ms_per_step"] - res["plain"]["ms_per_step"]
        res["window_spread_ms"] = {t: max(r.ms) - min(r.ms) for t, r in runs.items()}
    else:
        res["value"] = res[tags[0]]["ms_per_step"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
