#!/usr/bin/env python3
"""The bf16 AdamW kernel, the master-weights kernel and the stochastic-rounding kernel in ONE process over SANA-1.6B-sized flat
buffers, each alone on the chip.

    python scripts/adamw_master_bench.py [--n PARAMS] [--rounds R] [--steps K] [--out FILE.json]

Bytes per parameter (what the algorithm reads and writes, no gradient clear):
    bf16 step (yat_adamw_step)            14 = read p, g, m, v (2 B each) + write p, m, v;            18 with the EMA shadow
    master step (yat_adamw_master_step)   28 = read g (2) + master, m, v (4 each) + write them + p (2);  36 with the EMA shadow
    sr step (yat_adamw_sr_step)           14 = the bf16 step's traffic, + Philox4x32 in registers;       18 with the EMA shadow
The bf16 kernel's figure of the same run is the yardstick for the other two: all stream 16-byte accesses with no reuse.
The forms alternate over the rounds (one box, one process), every form warmed up first; device events bracket K launches."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from yat_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1604462752, help="parameters (default: SANA-1.6B's flat buffer)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, dev = a.n // 8 * 8, "cuda"
assert torch.cuda.is_available(), "this measurement needs the GPU"

gen = torch.Generator(device=dev).manual_seed(0)
p0 = (torch.randn(n, device=dev, generator=gen) * 0.02).to(torch.bfloat16)
gr = (torch.randn(n, device=dev, generator=gen) * 0.01).to(torch.bfloat16)
coef = torch.ones(1, device=dev)
HYP = (1e-5, 0.9, 0.999, 1e-8, 0.0)


def bf16_form(ema):
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    s = p.clone() if ema else None
    return (lambda step: ops.adamw_step(p, gr, m, v, coef, *HYP, step, zero_grad=False, ema_shadow=s, ema_decay=0.999)), p


def master_form(ema):
    p, w = p0.clone(), p0.float()
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    s = w.clone() if ema else None
    return (lambda step: ops.adamw_master_step(p, w, gr, m, v, coef, *HYP, step, zero_grad=False, ema_shadow=s, ema_decay=0.999)), p


def sr_form(ema):
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    s = p.clone() if ema else None
    return (lambda step: ops.adamw_sr_step(p, gr, m, v, coef, *HYP, step, zero_grad=False, ema_shadow=s, ema_decay=0.999, seed=0,
                                           rng_step=step, elem_offset=0)), p


FORMS = [("bf16", 14, bf16_form, False), ("master", 28, master_form, False), ("sr", 14, sr_form, False),
         ("bf16_ema", 18, bf16_form, True), ("master_ema", 36, master_form, True), ("sr_ema", 18, sr_form, True)]
results = {}
built = {name: make(ema) for name, _, make, ema in FORMS}      # ~110 GB at the default size, all six forms resident
step = 0
for name in built:                          # warm-up: code objects loaded, every buffer touched
    for _ in range(2):
        step += 1
        built[name][0](step)
torch.cuda.synchronize()
times = {name: [] for name in built}
for _ in range(a.rounds):
    for name in built:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step += 1
            built[name][0](step)
        e1.record()
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / a.steps)
for name, bpp, _, _ in FORMS:
    ms = sorted(times[name])
    best, med = ms[0], ms[len(ms) // 2]
    results[name] = {"bytes_per_param": bpp, "ms_per_launch_median": round(med, 4), "ms_per_launch_min": round(best, 4),
                     "ms_per_launch_all": [round(x, 4) for x in times[name]], "TB_per_s_median": round(bpp * n / med / 1e9, 3),
                     "checksum": built[name][1].float().sum().item()}
    print(f"{name:11s} {bpp} B/param: {med:.3f} ms median of {len(ms)} rounds x {a.steps} launches  {bpp * n / med / 1e9:.3f} TB/s")
out = {"params": n, "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "launches_per_round": a.steps, "forms": results,
       "master_over_bf16": round(results["master"]["TB_per_s_median"] / results["bf16"]["TB_per_s_median"], 3),
       "master_ema_over_bf16_ema": round(results["master_ema"]["TB_per_s_median"] / results["bf16_ema"]["TB_per_s_median"], 3),
       "master_ema_over_bf16": round(results["master_ema"]["TB_per_s_median"] / results["bf16"]["TB_per_s_median"], 3),
       "sr_over_bf16": round(results["sr"]["TB_per_s_median"] / results["bf16"]["TB_per_s_median"], 3),
       "sr_ema_over_bf16_ema": round(results["sr_ema"]["TB_per_s_median"] / results["bf16_ema"]["TB_per_s_median"], 3)}
print(f"master / bf16 bytes per second: {out['master_over_bf16']:.3f} (bar of the design: 0.85); with EMA against the plain bf16 "
      f"kernel: {out['master_ema_over_bf16']:.3f}")
print(f"sr / bf16 bytes per second: {out['sr_over_bf16']:.3f} (same bar); with EMA against the bf16 kernel with EMA: "
      f"{out['sr_ema_over_bf16_ema']:.3f}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
