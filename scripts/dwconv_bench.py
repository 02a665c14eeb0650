#!/usr/bin/env python3
"""Micro-benchmark of the GLU depthwise-conv kernels, by default at SANA-1.6B shapes (B=8, Hc=5600) for each aspect bucket.
Prints per-call times and sha1 digests of every output (to compare kernel variants or two builds through YAT_HIP_LIB bit for
bit; parity itself lives in tests/).

    python scripts/dwconv_bench.py [--shapes B,h,w,Hc ...] [--iters N] [--hash-only]
"""
import argparse, hashlib, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from yat_amd import ops
BF = torch.bfloat16
dev = "cuda"

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["8,32,32,5600", "8,16,64,5600", "8,24,42,5600", "8,44,22,5600"],
                help="B,h,w,Hc per shape (e.g. the dispatch-class shapes of tests/test_kernels_gpu.py)")
ap.add_argument("--iters", type=int, default=10, help="calls per timed window")
ap.add_argument("--hash-only", action="store_true", help="digests only, no timing")
args = ap.parse_args()

def timeit(fn, n=args.iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3

def sha(*ts):
    h = hashlib.sha1()
    for t in ts: h.update(t.contiguous().view(torch.int16).cpu().numpy().tobytes())
    return h.hexdigest()[:12]

g = torch.Generator(device=dev).manual_seed(0)
for B, h, w, Hc in (tuple(int(v) for v in s.split(",")) for s in args.shapes):
    tag = f"dwconv {h:2d}x{w:2d}" + ("" if (B, Hc) == (8, 5600) else f" (B={B}, Hc={Hc})")
    M = B * h * w
    z = torch.randn(M, 2 * Hc, generator=g, device=dev).to(BF)
    s = torch.nn.functional.silu(z.float()).to(BF)
    wdw = (torch.randn(2 * Hc, 9, generator=g, device=dev) * 0.3).to(BF)
    bdw = (torch.randn(2 * Hc, generator=g, device=dev) * 0.1).to(BF)
    dy = torch.randn(M, Hc, generator=g, device=dev).to(BF)
    y = torch.empty(M, Hc, dtype=BF, device=dev)
    dz = torch.empty(M, 2 * Hc, dtype=BF, device=dev)
    dw, db = torch.empty_like(wdw), torch.empty_like(bdw)
    ws = torch.empty(ops.dwconv_glu_bwd_workspace_bytes(B, h, w, Hc), dtype=torch.uint8, device=dev)
    u = torch.empty(M, 2 * Hc, dtype=BF, device=dev)
    du = torch.randn(M, 2 * Hc, generator=g, device=dev).to(BF)
    dzs = torch.empty(2 * Hc, dtype=BF, device=dev)
    fwd_u = lambda: ops.dwconv_glu_fwd(s, B, h, w, Hc, wdw, bdw, y, u_out=u)       # the step's configuration: keeps u
    bwd_du = lambda: ops.dwconv_glu_bwd(s, z, B, h, w, Hc, wdw, bdw, None, dz, dw, db, ws, dz_colsum=dzs, du=du)   # pass 2 only
    bwd_dy = lambda: ops.dwconv_glu_bwd(s, z, B, h, w, Hc, wdw, bdw, dy, dz, dw, db, ws, dz_colsum=dzs)
    fwd_u()
    print(f"{tag}: sha1(y,u)={sha(y, u)}")
    for name, call in (("du", bwd_du), ("dy", bwd_dy)):
        for t in (dz, dw, db, dzs): t.fill_(float("nan"))
        call()
        print(f"{tag}: bwd({name} given) sha1 dz={sha(dz)} dW={sha(dw)} db={sha(db)} dz_colsum={sha(dzs)}", flush=True)
    if args.hash_only:
        continue
    fu, b2 = timeit(fwd_u), timeit(bwd_du)
    print(f"{tag}: in-step config  fwd+u={fu:7.1f}us ({(M * 2 * Hc * 2 + M * Hc) * 2 / fu / 1e6:5.2f} TB/s)  "
          f"bwd2(du given)={b2:7.1f}us ({(M * 2 * Hc * 4) * 2 / b2 / 1e6:5.2f} TB/s)", flush=True)
    f = timeit(lambda: ops.dwconv_glu_fwd(s, B, h, w, Hc, wdw, bdw, y))
    b_ = timeit(lambda: ops.dwconv_glu_bwd(s, z, B, h, w, Hc, wdw, bdw, dy, dz, dw, db, ws))
    alg_f = (M * 2 * Hc + M * Hc) * 2
    alg_b = (M * 2 * Hc * 2 + M * Hc + M * 2 * Hc * 2 + M * 2 * Hc) * 2      # bwd1: s,dy -> du ; bwd2: du,s,z -> dz
    print(f"{tag}: fwd={f:7.1f}us ({alg_f / f / 1e6:5.2f} TB/s)  bwd={b_:7.1f}us ({alg_b / b_ / 1e6:5.2f} TB/s)  "
          f"chk y={y.float().sum().item():.3f} dz={dz.float().sum().item():.3f} dw={dw.float().sum().item():.3f} "
          f"db={db.float().sum().item():.3f}", flush=True)
