#!/usr/bin/env python3
"""gate backward, LayerNorm-modulate forward / backward (rows, cols), the column sum and the q|k RMSNorm backward on the SANA
activation shape (8 x 1024 x 2240), the caption RMSNorm forward / backward on 8 x 300 text rows x 2240: microseconds and GB/s
of the algorithmic bytes, alone on the chip.  ``YAT_HIP_LIB`` selects the library."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from yat_amd import ops
BF, dev = torch.bfloat16, "cuda"
B, N, D = 8, 1024, 2240
M = B * N
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(BF)
x, dy, lin, dres = rn(M, D), rn(M, D), rn(M, D), rn(M, D)
mod = rn(B, 6 * D)
dlin, dx, y = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
acc = torch.zeros(B, 6 * D, device=dev)
ws_g = torch.empty(int(ops._lib().yat_gate_bwd_workspace_bytes(M, D, N)), dtype=torch.uint8, device=dev)
ws_l = torch.empty(ops.ln_bwd_workspace_bytes(M, D, N), dtype=torch.uint8, device=dev)
dbias = torch.zeros(D, dtype=BF, device=dev)
mean = torch.empty(M, device=dev); rstd = torch.empty(M, device=dev)
ws_c = torch.empty(int(ops._lib().yat_colsum_workspace_bytes(M, D)), dtype=torch.uint8, device=dev)
dcol = torch.zeros(D, dtype=BF, device=dev)
# caption norm: yat_rmsnorm_fwd / _bwd on the text rows
Mt = 8 * 300
xt, dyt, yt, dxt = rn(Mt, D), rn(Mt, D), torch.empty(Mt, D, dtype=BF, device=dev), torch.empty(Mt, D, dtype=BF, device=dev)
wn, dwn = rn(D), torch.zeros(D, dtype=BF, device=dev)
rstd_t = torch.empty(Mt, device=dev)
ws_r = torch.empty(int(ops._lib().yat_rmsnorm_bwd_workspace_bytes(Mt, D)), dtype=torch.uint8, device=dev)
# q|k norm backward: two segments per row of a compact [M, 2D] matrix
x2, dy2, dx2 = rn(M, 2 * D), rn(M, 2 * D), torch.empty(M, 2 * D, dtype=BF, device=dev)
w2, dw2 = [rn(D), rn(D)], [torch.zeros(D, dtype=BF, device=dev) for _ in range(2)]
rstd2 = torch.rsqrt(x2.float().view(M, 2, D).pow(2).mean(-1) + 1e-5).contiguous()
ws_s = torch.empty(ops.rmsnorm_seg_bwd_workspace_bytes(M, D, 2), dtype=torch.uint8, device=dev)

def timed(f, n=30):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3

act = M * D * 2
cases = [
    ("gate_bwd (+bias)", lambda: ops.gate_bwd(dy, lin, mod[:, :D], 6 * D, N, dlin, acc[:, :D], 6 * D, ws_g, dbias), 3 * act),
    ("gate_bwd", lambda: ops.gate_bwd(dy, lin, mod[:, :D], 6 * D, N, dlin, acc[:, :D], 6 * D, ws_g), 3 * act),
    ("ln_fwd", lambda: ops.ln_modulate_fwd(x, mod[:, D:2 * D], mod[:, 2 * D:3 * D], 6 * D, N, 1e-6, y, mean, rstd), 2 * act),
    ("ln_bwd rows", lambda: ops.ln_modulate_bwd(x, mean, rstd, mod[:, 2 * D:3 * D], 6 * D, N, dy, dres, dx, acc[:, D:2 * D], acc[:, 2 * D:3 * D], 6 * D, ws_l, parts=1), 4 * act),
    ("ln_bwd cols", lambda: ops.ln_modulate_bwd(x, mean, rstd, mod[:, 2 * D:3 * D], 6 * D, N, dy, dres, dx, acc[:, D:2 * D], acc[:, 2 * D:3 * D], 6 * D, ws_l, parts=2), 2 * act),
    ("colsum", lambda: ops.colsum(dy, dcol, ws_c), act),
    ("rmsnorm_fwd text", lambda: ops.rmsnorm_fwd(xt, wn, 1e-5, y=yt, rstd=rstd_t), 2 * Mt * D * 2),
    ("rmsnorm_bwd text", lambda: ops.rmsnorm_bwd(xt, wn, rstd_t, dyt, dxt, dwn, ws_r), 3 * Mt * D * 2),
    ("rmsnorm_seg_bwd 2", lambda: ops.rmsnorm_seg_bwd(x2, w2, rstd2, dy2, dx2, dw2, ws_s), 3 * 2 * act),
]
for name, f, nbytes in cases:
    us = timed(f)
    print(f"{name:18s} {us:7.1f} us  {nbytes / us / 1e3:6.0f} GB/s")
print("checks", dlin.float().sum().item(), acc.sum().item(), dbias.float().sum().item(), dx.float().sum().item(),
      dcol.float().sum().item(), yt.float().sum().item(), dxt.float().sum().item(), dwn.float().sum().item(), dx2.float().sum().item())
