#!/usr/bin/env python3
"""FourierFT beside plain LoRA on the SANA-1.6B training step, and the two sparse kernels alone.

    python scripts/bench_fourierft.py [--batch 32] [--steps 8] [--warmup 3] [--alpha 0.01] [--out profiles/fourierft_a_bench.json]

One call measures, on one GPU:
* the B = 32 step (1024 px bucket 32 x 32 latents, prompts of 20..300 tokens, clip + AdamW) with ``fourierft_alpha`` adapters
  and with plain LoRA rank 8 on the README target modules, the same loop for both (recipe.optimize, backward, FlatAdamW.step);
* the adapter set's own share of the FourierFT step, split into expand / GEMM / contract: ``materialize()`` and ``project()``
  over all targets timed on an otherwise idle GPU, and the same loops with only the sparse kernels;
* ``yat_fourier_expand`` and ``yat_fourier_contract`` alone at 2240 x 11200 and 2240 x 2240 with n = alpha * out * in.
Times are medians of CUDA-event intervals; the result is one JSON object (also printed as one line)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16
TARGETS = ["conv_inverted", "conv_point", "to_q", "to_k", "to_v", "to_out.0", "linear_1", "linear_2", "proj"]


def timed(fn, reps, warmup=1):
    """median milliseconds of ``fn()`` over ``reps`` runs"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def step_time(make_adapters, args):
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    from yat_amd.recipe import SanaRecipe
    from yat_amd.optim import FlatAdamW
    cfg = SanaConfig(num_layers=args.layers)
    model = SanaTransformer2DModelHIP(cfg, device="cuda").init_synthetic(seed=0)
    ad = make_adapters(model)
    opt = FlatAdamW(ad, lr=1e-5, weight_decay=0.0, max_grad_norm=1.0)
    recipe = SanaRecipe(model, pad_to=512, device="cuda")
    g = torch.Generator().manual_seed(1234)
    latents = (torch.randn(args.batch, cfg.in_channels, 32, 32, generator=g) * 0.5).to(BF)
    embs = [torch.randn(int(L), cfg.caption_channels, generator=g).to(BF)
            for L in torch.randint(20, 301, (args.batch,), generator=g)]
    model.train()
    state = {}

    def step():
        loss, _, _ = recipe.optimize(latents, embs, torch.Generator().manual_seed(3), return_pred=True)
        loss.backward()
        opt.step()
        state["loss"] = loss

    ms = timed(step, args.steps, args.warmup)
    out = dict(ms_per_step=ms, images_per_s=1000.0 * args.batch / ms, loss=float(state["loss"].detach()),
               trainable_parameters=ad.num_parameters(), hbm_peak_gb=torch.cuda.max_memory_allocated() / 2 ** 30)
    return out, model, ad


def fourierft_split(ad, reps):
    """the adapter set's launches alone: whole materialize() / project(), and only their sparse kernels"""
    from yat_amd import ops
    for e in ad.entries:
        e["has_grad"] = True

    def expand_only():
        for e in ad.entries:
            csr, table, _, y = ad._plan(e)
            ops.fourier_expand(*csr, ad._views(e, ad.flat_param)[1], ad._s(e), table, y)

    def contract_only():
        for e in ad.entries:
            csr, table, _, z = ad._plan(e)
            ops.fourier_contract(*csr, z, ad._s(e), table, ad._views(e, ad.flat_grad)[1])

    def project():
        for e in ad.entries:
            e["has_grad"] = True
        ad.project()

    m, x, p, c = timed(ad.materialize, reps), timed(expand_only, reps), timed(project, reps), timed(contract_only, reps)
    return dict(materialize_ms=m, expand_ms=x, materialize_gemm_ms=m - x, project_ms=p, contract_ms=c, project_gemm_ms=p - c,
                targets=len(ad.entries), coefficients=ad.num_parameters())


def kernels_alone(out_dim, in_dim, alpha, reps):
    from yat_amd import ops
    from yat_amd.fourierft import build_csr, n_from_alpha, norm_factor, positions, twiddle_table
    n = n_from_alpha(alpha, out_dim, in_dim)
    u, v = positions(out_dim, in_dim, n)
    csr = tuple(t.cuda() for t in build_csr(u, v, out_dim, in_dim))
    rows, cols = min(out_dim, in_dim), max(out_dim, in_dim)
    table = twiddle_table(cols).cuda()
    g = torch.Generator().manual_seed(0)
    c = torch.randn((n + 7) // 8 * 8, generator=g).to(BF).cuda()
    y = torch.empty(2 * rows, cols, dtype=BF, device="cuda")
    dc = torch.zeros_like(c)
    s = norm_factor("ortho", out_dim, in_dim)
    ex = timed(lambda: ops.fourier_expand(*csr, c, s, table, y), reps)
    co = timed(lambda: ops.fourier_contract(*csr, y, s, table, dc), reps)
    gathers = float(n) * cols
    return dict(out=out_dim, inn=in_dim, n=n, expand_ms=ex, contract_ms=co, gathered_complex_macs=gathers,
                expand_gmacs_per_s=gathers / ex / 1e6, contract_gmacs_per_s=gathers / co / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=20, help="debug only; anything but 20 is not SANA-1.6B")
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fourierft_a_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fourierft.py needs a GPU (the HIP path has no CPU fallback)")
    from yat_amd.fourierft import FourierFTAdapters
    from yat_amd.lora import LoRAAdapters
    res = dict(workload=f"SANA-1.6B ({args.layers} blocks) 1024px bf16 step, B = {args.batch}, 32 x 32 latents, adapters on "
                        f"{TARGETS}", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup)
    res["kernels_alone"] = [kernels_alone(2240, 11200, args.alpha, 5), kernels_alone(2240, 2240, args.alpha, 5)]
    print(json.dumps(res["kernels_alone"]), flush=True)
    fft, model, ad = step_time(lambda m: FourierFTAdapters(m, TARGETS, alpha=args.alpha), args)
    res["fourierft"] = dict(fft, alpha=args.alpha, split=fourierft_split(ad, 3))
    print(json.dumps(res["fourierft"]), flush=True)
    del model, ad
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    lora, model, ad = step_time(lambda m: LoRAAdapters(m, TARGETS, r=8, alpha=8.0), args)
    res["lora_r8"] = lora
    sp = res["fourierft"]["split"]
    sparse = sp["expand_ms"] + sp["contract_ms"]
    res["summary"] = dict(fourierft_ms=fft["ms_per_step"], lora_r8_ms=lora["ms_per_step"], expand_ms=sp["expand_ms"],
                          gemm_ms=sp["materialize_gemm_ms"] + sp["project_gemm_ms"], contract_ms=sp["contract_ms"],
                          rest_ms=fft["ms_per_step"] - sp["materialize_ms"] - sp["project_ms"],
                          sparse_share=sparse / fft["ms_per_step"])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
