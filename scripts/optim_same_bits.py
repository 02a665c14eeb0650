#!/usr/bin/env python3
"""Same-bits listing of the optimizer kernels (csrc/optim.hip): one SHA-1 per output buffer, on seeded inputs.

    python scripts/optim_same_bits.py > listing.txt

The script drives the ``yat_amd`` package of the tree it lies in and uses only ``ops`` calls whose Python signature does not
change between commits, so the same file, copied into a ``git worktree`` of another commit, gives that commit's listing; two
commits compute the same bits when ``cmp`` finds the two listings identical.

Norm: the three edge layouts of tests/test_optim_gpu.py (EDGE_LAYOUTS, restated here) through ``gradnorm_pieces_partial``
without and with an ``owned`` mask + ``gradnorm_pieces_finish``, and through ``gradnorm_clip``: every partial slot, the norm and
the coefficient at max_norm 1.0 and 1e5, and once with a NaN among the gradients.
Steps: ``adamw_step``, ``adamw_master_step`` and ``adamw_sr_step`` (at ``elem_offset`` 0 and 8 x 1237) at n = 8, 8 x 257 and
2^24 + 8 x 1001 (one pass of the capped grid plus an odd tail), with and without a clip coefficient, with and without the
shadow, weight decay 0 and 0.01, three consecutive steps; one case per step with NaN and +-inf gradients."""
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from yat_amd import ops  # noqa: E402
from yat_amd.optim import norm_pieces  # noqa: E402

BF, DEV = torch.bfloat16, "cuda"
CHUNK = 1 << 18
EDGE_LAYOUTS = {
    "eighths": ([[1, 7, 8], [CHUNK - 1, 0, CHUNK], [CHUNK + 1, 3 * CHUNK + 5], [20 * CHUNK + 3, 8]], True),
    "eighths_tail": ([[1, 7, 8, CHUNK - 1], [0, CHUNK, 20 * CHUNK + 3], [CHUNK + 1, 3 * CHUNK + 5]], False),
    "whole": ([[1, 7, 8, CHUNK - 1, 0, CHUNK, CHUNK + 1, 20 * CHUNK + 3, 3 * CHUNK + 5]], False),
}


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha1(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def emit(name, t):
    print(f"{sha(t)}  {name}  [{t.numel()} {str(t.dtype).replace('torch.', '')}]", flush=True)


def _up(x, a):
    return -(-x // a) * a


def edge_layout(buckets, pad_end):
    seg, lens, lows, off = [], [], [], 0
    for lens_b in buckets:
        off = _up(off, 64)
        lows.append(off)
        for L in lens_b:
            seg.append(off)
            lens.append(L)
            off += _up(L, 8)
    n = _up(off, 64) if pad_end else seg[-1] + lens[-1]
    return seg + [n], lens, list(zip(lows, lows[1:] + [n]))


def norm_cases():
    for layout, spec in EDGE_LAYOUTS.items():
        seg, lens, bounds = edge_layout(*spec)
        n, nt = seg[-1], len(lens)
        gen = torch.Generator().manual_seed(31)
        g_cpu = torch.zeros(n, dtype=BF)
        for i, (s, L) in enumerate(zip(seg, lens)):
            g_cpu[s:s + L] = (torch.randn(L, generator=gen) * 4.0 ** (i % 5 - 2)).to(BF)
        ps, tf, cb, mx, _ = norm_pieces(seg, bounds)
        ps_d = torch.tensor(ps, dtype=torch.int64, device=DEV)
        tf_d, cb_d = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in (tf, cb))
        seg_d = torch.tensor(seg, dtype=torch.int64, device=DEV)
        owned = torch.tensor([p % 3 != 1 for p in range(len(ps) - 1)], dtype=torch.uint8, device=DEV)
        for poison in (False, True):
            g = g_cpu.to(DEV)
            if poison:
                g[seg[-2] + lens[-1] // 2] = float("nan")
            tag = f"norm {layout}{' NaN' if poison else ''}"
            for mask_name, mask in (("all", None), ("owned", owned)):
                partial = torch.full((cb[-1],), float("nan"), device=DEV)
                ops.gradnorm_pieces_partial(g, ps_d, cb_d, mx, mask, partial)
                emit(f"{tag} pieces {mask_name}: partial", partial)
                for max_norm in (1.0, 1e5):
                    norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
                    ops.gradnorm_pieces_finish(tf_d, cb_d, partial, max_norm, norm, coef)
                    emit(f"{tag} pieces {mask_name} max_norm={max_norm:g}: norm", norm)
                    emit(f"{tag} pieces {mask_name} max_norm={max_norm:g}: coef", coef)
            for max_norm in (1.0, 1e5):
                ws = torch.full((ops.gradnorm_workspace_bytes(n, nt) // 4,), float("nan"), device=DEV)
                norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
                ops.gradnorm_clip(g, seg_d, max_norm, norm, coef, ws)
                emit(f"{tag} per-tensor max_norm={max_norm:g}: workspace", ws)
                emit(f"{tag} per-tensor max_norm={max_norm:g}: norm", norm)
                emit(f"{tag} per-tensor max_norm={max_norm:g}: coef", coef)


HYP = (3e-4, 0.9, 0.999, 1e-8)         # lr, beta1, beta2, eps
KINDS = (("bf16", 0), ("master", 0), ("sr", 0), ("sr", 8 * 1237))


def step_case(kind, elem_offset, src, clip, shadow, wd, tag):
    p, gr, m, v = (t.to(DEV) for t in src)
    coef = torch.full((1,), 0.37, dtype=torch.float32, device=DEV) if clip else None
    if kind == "master":
        w, m, v = p.float(), m.float(), v.float()
        s = w.clone() if shadow else None
    else:
        s = p.clone() if shadow else None
    for step in (1, 2, 3):
        kw = dict(zero_grad=False, ema_shadow=s, ema_decay=0.999)
        if kind == "bf16":
            ops.adamw_step(p, gr, m, v, coef, *HYP, wd, step, **kw)
        elif kind == "master":
            ops.adamw_master_step(p, w, gr, m, v, coef, *HYP, wd, step, **kw)
        else:
            ops.adamw_sr_step(p, gr, m, v, coef, *HYP, wd, step, **kw, seed=0x1234567890ABCDEF, rng_step=step + 40,
                              elem_offset=elem_offset)
    out = [("param", p), ("exp_avg", m), ("exp_avg_sq", v), ("grad", gr)]
    if kind == "master":
        out.append(("master", w))
    if shadow:
        out.append(("shadow", s))
    for name, t in out:
        emit(f"{tag}: {name}", t)


def step_cases():
    for n in (8, 8 * 257, (1 << 24) + 8 * 1001):
        gen = torch.Generator().manual_seed(1000 + n % 997)
        src = [(torch.randn(n, generator=gen) * sc).to(BF) for sc in (0.02, 1e-3, 1e-3, 1e-6)]
        src[3].abs_()
        for (kind, off), clip, shadow, wd in itertools.product(KINDS, (True, False), (True, False), (0.0, 0.01)):
            step_case(kind, off, src, clip, shadow, wd,
                      f"step {kind} n={n} elem_offset={off} clip={int(clip)} shadow={int(shadow)} wd={wd:g}")
    n = 8 * 257
    gen = torch.Generator().manual_seed(77)
    src = [(torch.randn(n, generator=gen) * sc).to(BF) for sc in (0.02, 1e-3, 1e-3, 1e-6)]
    src[3].abs_()
    for i, bad in enumerate((float("nan"), float("inf"), float("-inf"))):
        src[1][i::97] = bad
    for kind, off in KINDS:
        step_case(kind, off, src, True, True, 0.01, f"step {kind} n={n} elem_offset={off} NaN / +-inf gradients")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this listing needs the GPU"
    norm_cases()
    step_cases()
