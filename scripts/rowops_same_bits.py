#!/usr/bin/env python3
"""Same-bits check of the row and strip kernels (csrc/rowops.hip) and of one tiny SANA step between two builds.

    YAT_HIP_LIB=PARENT/yat_amd/libyat_hip.so python scripts/rowops_same_bits.py --out parent.pt
    python scripts/rowops_same_bits.py --out work.pt                                              # this tree's own library
    python scripts/rowops_same_bits.py --compare parent.pt work.pt --allow 'rmsnorm_bwd * dw*' 'tiny sana grad caption_norm.weight'

``YAT_HIP_LIB`` selects the library; this tree's ``yat_amd`` package drives both (the C ABI is the same).  On seeded inputs,
at one test-sized shape and at the step's shape (8192 x 2240; the caption norm: 2400 x 2240), the outputs of ``rmsnorm_fwd`` /
``rmsnorm_bwd``, ``rmsnorm_seg_fwd`` / ``_bwd`` (one and two segments, with and without dw), ``colsum`` and ``gate_bwd``
(plain and accumulating, ``gate_bwd`` also without dbias) and ``ln_modulate_bwd`` (parts 1, 2, 3) are saved, and the loss and
every parameter gradient of one ``optimize_device`` step of the tiny SANA model of scripts/recipe_same_bits.py.  ``--compare``
prints one ``torch.equal`` verdict per entry.  Entries matching an ``--allow`` pattern (fnmatch) may differ: for those the number
of differing elements and the largest distance in bf16 ulps are printed.  Exit status 1 on any other difference."""
import argparse
import fnmatch
import os
import sys

import torch

BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-5


def randn(*shape, seed, gain=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * gain).to(BF).cuda()


def wspace(nbytes):
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device="cuda")


def run_rowops(out):
    from yat_amd import ops
    lib = ops._lib()

    for M, D in ((67, 72), (2400, 2240)):
        tag = f"{M} x {D}"
        x, dy, w, prior = randn(M, D, seed=1, gain=1.5), randn(M, D, seed=2), randn(D, seed=3, gain=0.3) + 1, randn(D, seed=4, gain=2.0)
        y, rstd = ops.rmsnorm_fwd(x, w, EPS)
        out[f"rmsnorm_fwd {tag} y"], out[f"rmsnorm_fwd {tag} rstd"] = y, rstd
        for acc in (False, True):
            dx, dw = torch.empty_like(x), prior.clone()
            ops.rmsnorm_bwd(x, w, rstd, dy, dx, dw, wspace(lib.yat_rmsnorm_bwd_workspace_bytes(M, D)), accumulate_dw=acc)
            out[f"rmsnorm_bwd {tag} acc={int(acc)} dx"], out[f"rmsnorm_bwd {tag} acc={int(acc)} dw"] = dx, dw

    for M, D in ((67, 72), (8192, 2240)):
        for nseg in (1, 2):
            tag = f"{M} x {nseg} x {D}"
            x, dy = randn(M, nseg * D, seed=5, gain=1.5), randn(M, nseg * D, seed=6)
            ws_ = [randn(D, seed=7 + s, gain=0.3) + 1 for s in range(nseg)]
            y, keep, rstd = torch.empty_like(x), torch.empty_like(x), torch.empty(M, nseg, device="cuda")
            ops.rmsnorm_seg_fwd(x, ws_, EPS, y, rstd, keep=keep)
            out[f"rmsnorm_seg_fwd {tag} y"], out[f"rmsnorm_seg_fwd {tag} rstd"], out[f"rmsnorm_seg_fwd {tag} keep"] = y, rstd, keep
            for mode in ("no dw", "dw", "dw accumulated"):
                dx = torch.empty_like(x)
                dws = None if mode == "no dw" else [randn(D, seed=9 + s, gain=2.0) for s in range(nseg)]
                ops.rmsnorm_seg_bwd(x, ws_, rstd, dy, dx, dws, None if dws is None else wspace(ops.rmsnorm_seg_bwd_workspace_bytes(M, D, nseg)),
                                    accumulate_dw=mode == "dw accumulated")
                out[f"rmsnorm_seg_bwd {tag} {mode}: dx"] = dx
                for s, t in enumerate(dws or ()):
                    out[f"rmsnorm_seg_bwd {tag} {mode}: dw{s}"] = t

    for rows, cols in ((300, 520), (8192, 2240)):
        x = randn(rows, cols, seed=11)
        for acc in (False, True):
            o = randn(cols, seed=12, gain=2.0)
            ops.colsum(x, o, wspace(lib.yat_colsum_workspace_bytes(rows, cols)), accumulate=acc)
            out[f"colsum {rows} x {cols} acc={int(acc)}"] = o

    for B, rpb, D in ((3, 130, 264), (8, 1024, 2240)):
        M, tag = B * rpb, f"{B} x {rpb} x {D}"
        dout, lin, mod = randn(M, D, seed=13), randn(M, D, seed=14), randn(B, 6, D, seed=15)
        for mode in ("no dbias", "dbias", "dbias accumulated"):
            dlin, acc = torch.empty_like(dout), randn(B, 6, D, seed=16).float()
            dbias = None if mode == "no dbias" else randn(D, seed=17, gain=2.0)
            ops.gate_bwd(dout, lin, mod[:, 5], 6 * D, rpb, dlin, acc[:, 5], 6 * D, wspace(lib.yat_gate_bwd_workspace_bytes(M, D, rpb)),
                         dbias=dbias, accumulate_bias=mode == "dbias accumulated")
            out[f"gate_bwd {tag} {mode}: dlin"], out[f"gate_bwd {tag} {mode}: dgate table"] = dlin, acc
            if dbias is not None:
                out[f"gate_bwd {tag} {mode}: dbias"] = dbias

        x, dy, dres = randn(M, D, seed=18, gain=2.0) + 0.5, randn(M, D, seed=19), randn(M, D, seed=20)
        _, mean, rstd = ops.ln_modulate_fwd(x, mod[:, 3], mod[:, 4], 6 * D, rpb, 1e-6)
        for parts in (1, 2, 3):
            dx, acc = torch.zeros_like(x), randn(B, 6, D, seed=21).float()
            ops.ln_modulate_bwd(x, mean, rstd, mod[:, 4], 6 * D, rpb, dy, dres, dx, acc[:, 3], acc[:, 4], 6 * D,
                                wspace(ops.ln_bwd_workspace_bytes(M, D, rpb)), parts=parts)
            out[f"ln_modulate_bwd {tag} parts={parts}: dx"], out[f"ln_modulate_bwd {tag} parts={parts}: dshift | dscale table"] = dx, acc


def run_tiny_sana(out):
    from yat_amd.recipe import SanaRecipe
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    cfg = SanaConfig(num_layers=2, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=2,
                     cross_attention_head_dim=64, cross_attention_dim=128, caption_channels=96, in_channels=8, out_channels=8,
                     sample_size=32)
    model = SanaTransformer2DModelHIP(cfg, device="cuda").init_synthetic(4)
    recipe = SanaRecipe(model, pad_to=128, device="cuda")
    g = torch.Generator().manual_seed(9)
    torch.manual_seed(21)
    torch.cuda.manual_seed(21)
    latents = (torch.randn(2, cfg.in_channels, 8, 8, generator=g) * 0.5).to(BF)
    embs = [torch.randn(L, 96, generator=g).to(BF) for L in (40, 128)]
    loss = recipe.optimize_device(latents, embs, torch.Generator().manual_seed(100), gscale=1.0)
    torch.cuda.synchronize()
    out["tiny sana loss"] = loss.detach()
    for name, grad in model.G.items():
        out[f"tiny sana grad {name}"] = grad


def run():
    out = {}
    run_rowops(out)
    run_tiny_sana(out)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def bf16_ulps(a, b):
    """largest distance between two bf16 tensors, counted in representable bf16 values"""
    def ordered(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7FFF), bits)
    return int((ordered(a) - ordered(b)).abs().max())


def compare(a_path, b_path, allow):
    a, b = torch.load(a_path), torch.load(b_path)
    ok = set(a) == set(b)
    differing = []
    for name in a:
        same = name in b and a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and torch.equal(a[name], b[name])
        finite = bool(torch.isfinite(a[name].float()).all())
        allowed = any(fnmatch.fnmatchcase(name, pat) for pat in allow)
        line = f"{name}: {'EQUAL' if same else 'DIFFERENT'} ({a[name].numel()} elements{'' if finite else ', NOT finite'})"
        if not same and name in b and a[name].shape == b[name].shape and a[name].dtype == BF:
            line += f": {int((a[name] != b[name]).sum())} elements differ, at most {bf16_ulps(a[name], b[name])} bf16 ulp"
        if not same:
            differing.append(name)
            line += " -- allowed to differ" if allowed else " -- NOT allowed"
        ok = ok and finite and (same or allowed)
        print(line)
    print(f"{len(a)} entries, {len(differing)} differ ({', '.join(differing) or 'none'}): "
          + ("every entry outside the allowed list is torch.equal" if ok else "FAILED"))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--allow", nargs="*", default=[], help="entry names (fnmatch patterns) that may differ")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare, args.allow))
    sys.path.insert(0, os.path.dirname(HERE))
    results = run()
    print(f"{len(results)} entries with {os.environ.get('YAT_HIP_LIB') or 'the tree library'}", flush=True)
    torch.save(results, args.out)


if __name__ == "__main__":
    main()
