#!/usr/bin/env python3
"""Micro-benchmark of the adapter kernels (csrc/lokr.hip) at the sizes of the B = 32 step (M = 32768 tokens), one line per kernel
with its time and its rate against the HBM traffic it cannot avoid:
  the LoKr row products  T1 = x' w2_b^T (forward, plain and flat layouts) and dx' += H' w2_b,
  rank_expand            R = 8 and 64, both forms, N = 2240,
  lokr_small_wgrad       R = 8 at N = 56 over M * 40 rows, R = 64 at N = 2240 over M rows,
  hadamard_scale / _bwd and dora_delta / _bwd at 2240 x 2240.
Warm = back-to-back launches on the same buffers (whatever fits stays in the Infinity Cache); cold = every launch after a
1 GiB fill, the fill's own time subtracted.  YAT_HIP_LIB selects the library (scripts/build_variant.py)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from yat_amd import ops
BF, dev = torch.bfloat16, "cuda"


def timeit(fn, n=20):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


M = 32768
junk = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
tj = timeit(lambda: junk.fill_(1))


def cold(fn):
    def run():
        junk.fill_(1); fn()
    return run


def line(name, mb, fn):
    """one kernel: warm and cold microseconds, TB/s of its ``mb`` megabytes at the warm time"""
    w, c = timeit(fn), timeit(cold(fn)) - tj
    print(f"{name}: {w:7.1f} us ({mb / w:5.2f} TB/s; cold {c:7.1f} us, {mb / c:5.2f} TB/s)", flush=True)


def mbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors) / 1e6


for K, im, n_ in ((2240, 40, 56), (5600, 70, 80), (11200, 100, 112)):
    R = 8
    x = torch.randn(M * im, n_, device=dev).to(BF)
    wb = (torch.randn(R, n_, device=dev) * 0.3).to(BF)
    t1 = torch.empty(M * im, R, dtype=BF, device=dev)
    slab = torch.zeros(M, K, dtype=BF, device=dev)
    h = torch.randn(M * im, R, device=dev).to(BF)
    dx = torch.randn(M * im, n_, device=dev).to(BF)
    tag = f"K={K} in_m={im} in_n={n_}"
    line(f"lokr_rows fwd {tag}", mbytes(x, t1), lambda: ops.lokr_rows_fwd(x, wb, t1))
    line(f"lokr_rows_fwd_flat {tag}", mbytes(x, t1), lambda: ops.lokr_rows_fwd_flat(x, wb, slab[:, :im * R], im))
    line(f"lokr_rows bwd {tag}", mbytes(dx, dx, h), lambda: ops.lokr_rows_bwd(h, wb, dx))
    if K == 2240:                                    # the rank-8 adapter gradient of the same target: d_w2_b = H'^T x'
        g = torch.empty(R, n_, dtype=BF, device=dev)
        line(f"lokr_small_wgrad R=8 N={n_} rows={M * im}", mbytes(h, x), lambda: ops.lokr_small_wgrad(h, x, g))
    del x, t1, slab, h, dx

N = 2240
for R in (8, 64):
    h = torch.randn(M, R, device=dev).to(BF)
    w = (torch.randn(R, N, device=dev) * 0.3).to(BF)
    io = torch.zeros(M, N, dtype=BF, device=dev)     # (residual = 1 adds bf16(h w) to it launch after launch: zeros keep it finite)
    line(f"rank_expand R={R} N={N} rows={M} residual=0", mbytes(h, io), lambda: ops.rank_expand(h, w, io, scale=0.5))
    h.zero_()
    line(f"rank_expand R={R} N={N} rows={M} residual=1", mbytes(h, io, io), lambda: ops.rank_expand(h, w, io, residual=True))
    if R == 64:
        h, x, g = torch.randn(M, R, device=dev).to(BF), torch.randn(M, N, device=dev).to(BF), torch.empty(R, N, dtype=BF, device=dev)
        line(f"lokr_small_wgrad R={R} N={N} rows={M}", mbytes(h, x), lambda: ops.lokr_small_wgrad(h, x, g))

a, b, dd = (torch.randn(N, N, device=dev).to(BF) for _ in range(3))
o1, o2 = torch.empty_like(a), torch.empty_like(a)
line(f"hadamard_scale {N} x {N}", mbytes(a, b, o1), lambda: ops.hadamard_scale(a, b, 0.75, o1))
line(f"hadamard_bwd {N} x {N}", mbytes(dd, a, b, o1, o2), lambda: ops.hadamard_bwd(dd, a, b, 0.75, o1, o2))
mag, dmag = torch.rand(N, device=dev).to(BF) + 0.5, torch.empty(N, dtype=BF, device=dev)
s_buf, n_buf = torch.empty(N, device=dev), torch.empty(N, device=dev)
line(f"dora_delta {N} x {N}", mbytes(a, b, o1), lambda: ops.dora_delta(a, b, mag, 0.5, o1, s_buf, n_buf))
line(f"dora_bwd {N} x {N}", mbytes(dd, a, b, o1), lambda: ops.dora_bwd(dd, a, b, 0.5, s_buf, n_buf, o1, dmag))
