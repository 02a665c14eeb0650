#!/usr/bin/env python3
"""Same-bits check of the adapter kernels (csrc/lokr.hip) and of one tiny SANA step per adapter kind between two builds.

    YAT_HIP_LIB=PARENT/yat_amd/libyat_hip.so python scripts/adapter_kernels_same_bits.py --out parent.pt
    python scripts/adapter_kernels_same_bits.py --out work.pt                                     # this tree's own library
    python scripts/adapter_kernels_same_bits.py --compare parent.pt work.pt

``YAT_HIP_LIB`` selects the library; this tree's ``yat_amd`` package drives both (the C ABI is the same).  The kernel tests
use small-integer operands so that every sum is exact in any order -- which also means they cannot see a changed order of
summation.  Here the operands are seeded ``randn`` in bf16: at one test-sized shape and at the shape of the B = 32 step
(D = 2240: 32768 tokens, a 2240 x 2240 target factored 40 x 56) the outputs of all twelve entry points of the file are saved --
``lokr_delta``, ``lokr_project``, ``lokr_rows`` forward / backward, ``lokr_rows_fwd_flat``, ``lora_scatter_b``, ``rank_expand``
(both forms), ``lokr_small_wgrad`` (plain and accumulating), ``hadamard_scale`` / ``_bwd``, ``dora_delta`` / ``_bwd`` -- and the
loss and adapter gradients of one step of a tiny SANA model under LoKr, LoRA (r 8 and 64), LoHa and DoRA.  An output of more
than 2^20 elements is kept as the SHA-256 of its bytes.  ``--compare`` prints one ``torch.equal`` verdict per entry; there is no
list of entries that may differ.  Exit status 1 on any difference."""
import argparse
import hashlib
import os
import sys

import torch

BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
TARGETS = ["conv_inverted", "conv_point", "to_q", "to_k", "to_v", "to_out.0", "linear_1", "linear_2", "proj"]
M = 32768                                            # tokens of the B = 32 step


def randn(*shape, seed, gain=1.0, ld=None):
    """seeded bf16 randn on the device; with ``ld`` a [rows, cols] view with that row stride"""
    t = (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * gain).to(BF).cuda()
    if ld is None:
        return t
    buf = torch.zeros(shape[0], ld, dtype=BF, device="cuda")
    buf[:, :shape[1]].copy_(t)
    return buf[:, :shape[1]]


def run_kernels(out):
    from yat_amd import ops
    lib = ops._lib()

    # LoKr delta and its projection: (out_l, out_k, in_m, in_n, r, row stride)
    for ol, ok, im, inn, r, ld in ((3, 5, 2, 8, 2, 24), (40, 56, 40, 56, 8, 2240)):
        tag = f"{ol}x{ok} {im}x{inn} r{r}"
        w1, wa, wb = randn(ol, im, seed=1, gain=0.3), randn(ok, r, seed=2, gain=0.3), randn(r, inn, seed=3, gain=0.3)
        delta = torch.zeros(ol * ok, ld, dtype=BF, device="cuda")[:, :im * inn]
        ops.lokr_delta(w1, wa, wb, 0.5, delta)
        out[f"lokr_delta {tag}"] = delta
        dd = randn(ol * ok, im * inn, seed=4, ld=ld)
        g1, ga, gb = torch.empty_like(w1), torch.empty_like(wa), torch.empty_like(wb)
        ws = torch.empty(int(lib.yat_lokr_project_workspace_bytes(ol, ok, inn)), dtype=torch.uint8, device="cuda")
        ops.lokr_project(w1, wa, wb, 0.5, dd, g1, ga, gb, ws)
        out[f"lokr_project {tag} d_w1"], out[f"lokr_project {tag} d_w2_a"], out[f"lokr_project {tag} d_w2_b"] = g1, ga, gb

    # the row products with w2_b: (rows, in_m, N, R)
    for rows, im, N, R in ((1000, 5, 40, 16), (M * 40, 40, 56, 8)):
        tag = f"{rows} x {N} R{R}"
        x, wb, h = randn(rows, N, seed=5), randn(R, N, seed=6, gain=0.3), randn(rows, R, seed=7)
        out[f"lokr_rows fwd {tag}"] = ops.lokr_rows_fwd(x, wb, torch.empty(rows, R, dtype=BF, device="cuda"))
        slab = torch.zeros(rows // im, im * R + 64, dtype=BF, device="cuda")
        ops.lokr_rows_fwd_flat(x, wb, slab[:, :im * R], im)
        out[f"lokr_rows_fwd_flat {tag}"] = slab
        out[f"lokr_rows bwd {tag}"] = ops.lokr_rows_bwd(h, wb, x.clone())
        del x, h, slab

    # rank expansion and the small-output weight gradient: (rows, N, row stride, ranks)
    for rows, N, ld, ranks in ((67, 520, 528, (8, 16, 32, 64, 128)), (M, 2240, 2240, (8, 64))):
        for R in ranks:
            tag = f"{rows} x {N} R{R}"
            h, w = randn(rows, R, seed=8), randn(R, N, seed=9, gain=0.3)
            for residual in (0, 1):
                io = randn(rows, N, seed=10, ld=ld)
                out[f"rank_expand {tag} residual={residual}"] = ops.rank_expand(h, w, io, scale=2.0 / 3.0, residual=bool(residual))
            x = randn(rows, N, seed=11, ld=ld)
            for acc in (False, True):
                g = randn(R, N, seed=12, gain=4.0)
                ops.lokr_small_wgrad(h, x, g, accumulate=acc, scale=0.5)
                out[f"lokr_small_wgrad {tag} acc={int(acc)}"] = g
            del h, x, io
    rows, N, R = M * 40, 56, 8                                              # the rank-8, in_n = 56 adapter gradient of the step
    a, x, g = randn(rows, R, seed=13), randn(rows, N, seed=14), torch.empty(R, N, dtype=BF, device="cuda")
    ops.lokr_small_wgrad(a, x, g)
    out[f"lokr_small_wgrad {rows} x {N} R{R}"] = g
    del a, x

    # scaling * lora_B^T of every adapter into the shadow of the flat weights: [(out, in)], R
    for dims, R in ((((300, 64), (72, 136)), 8), (((2240, 2240),) * 4, 64)):
        src = randn(sum(R * o for o, _ in dims), seed=15)
        dst = torch.zeros(sum(o * i for o, i in dims), dtype=BF, device="cuda")
        table, so, do = [], 0, 0
        for o, i in dims:
            table.append([so, do, o, i])
            so, do = so + R * o, do + o * i
        ops.lora_scatter_b(torch.tensor(table, dtype=torch.int64, device="cuda"), len(dims), max(o for o, _ in dims), R, 0.25, src, dst)
        out[f"lora_scatter_b {len(dims)} x {dims[0]} R{R}"] = dst

    # LoHa and DoRA element-wise and row kernels: (rows, cols, row stride)
    for rows, cols, ld in ((33, 72, 80), (2240, 2240, 2240)):
        tag = f"{rows} x {cols}"
        a, b, dd = randn(rows, cols, seed=16, ld=ld), randn(rows, cols, seed=17, ld=ld), randn(rows, cols, seed=18, ld=ld)
        out[f"hadamard_scale {tag}"] = ops.hadamard_scale(a, b, 0.75, torch.zeros(rows, ld, dtype=BF, device="cuda")[:, :cols])
        t1, t2 = torch.zeros(rows, ld, dtype=BF, device="cuda")[:, :cols], torch.zeros(rows, cols, dtype=BF, device="cuda")
        ops.hadamard_bwd(dd, a, b, 0.75, t1, t2)
        out[f"hadamard_bwd {tag} t1"], out[f"hadamard_bwd {tag} t2"] = t1, t2
        mag = randn(rows, seed=19).abs() + 0.5
        delta = torch.zeros(rows, ld, dtype=BF, device="cuda")[:, :cols]
        s_buf, n_buf = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
        ops.dora_delta(a, b, mag, 0.5, delta, s_buf, n_buf)
        out[f"dora_delta {tag} delta"], out[f"dora_delta {tag} s"], out[f"dora_delta {tag} n"] = delta, s_buf, n_buf
        t1, dmag = torch.zeros(rows, ld, dtype=BF, device="cuda")[:, :cols], torch.empty(rows, dtype=BF, device="cuda")
        ops.dora_bwd(dd, a, b, 0.5, s_buf, n_buf, t1, dmag)
        out[f"dora_bwd {tag} t1"], out[f"dora_bwd {tag} dmag"] = t1, dmag


def run_tiny_sana(out):
    from yat_amd.dora import DoRAAdapters
    from yat_amd.loha import LoHaAdapters
    from yat_amd.lokr import LoKrAdapters
    from yat_amd.lora import LoRAAdapters
    from yat_amd.recipe import SanaRecipe
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    cfg = SanaConfig(num_layers=2, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=2,
                     cross_attention_head_dim=64, cross_attention_dim=128, caption_channels=96, in_channels=8, out_channels=8,
                     sample_size=32)
    kinds = (("lokr r2", LoKrAdapters, 2, 4.0), ("lora r8", LoRAAdapters, 8, 16.0), ("lora r64", LoRAAdapters, 64, 128.0),
             ("loha r2", LoHaAdapters, 2, 4.0), ("dora r4", DoRAAdapters, 4, 4.0))
    for tag, cls, r, alpha in kinds:
        torch.manual_seed(21)                        # (the adapters draw their initial values from the global streams)
        torch.cuda.manual_seed(21)
        model = SanaTransformer2DModelHIP(cfg, device="cuda").init_synthetic(4)
        ad = cls(model, TARGETS, r=r, alpha=alpha)
        g = torch.Generator().manual_seed(9)
        # every adapter parameter away from its zero init (the DoRA magnitudes stay near their row norms)
        ad.flat_param.add_((torch.randn(ad.flat_param.numel(), generator=g) * 0.05).to(BF).cuda())
        latents = (torch.randn(2, cfg.in_channels, 8, 8, generator=g) * 0.5).to(BF)
        embs = [torch.randn(L, 96, generator=g).to(BF) for L in (40, 128)]
        model.train()
        loss = SanaRecipe(model, pad_to=128, device="cuda").optimize(latents, embs, torch.Generator().manual_seed(100))
        loss.backward()
        torch.cuda.synchronize()
        out[f"tiny sana {tag} loss"], out[f"tiny sana {tag} adapter gradients"] = loss.detach(), ad.flat_grad


def keep(t):
    t = t.detach().contiguous().cpu()
    if t.numel() <= 1 << 20:
        return t.clone()
    return torch.frombuffer(bytearray(hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).digest()), dtype=torch.uint8).clone()


class Kept(dict):
    """outputs leave the device as they come (the step-sized ones are large)"""
    def __setitem__(self, name, t):
        torch.cuda.synchronize()
        super().__setitem__(name, keep(t))


def run():
    out = Kept()
    run_kernels(out)
    run_tiny_sana(out)
    return dict(out)


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    differing = [n for n in sorted(set(a) ^ set(b))]
    for name in a:
        same = name in b and a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and torch.equal(a[name], b[name])
        what = "SHA-256 of the output" if a[name].dtype == torch.uint8 else f"{a[name].numel()} elements"
        finite = a[name].dtype == torch.uint8 or bool(torch.isfinite(a[name].float()).all())
        print(f"{name}: {'EQUAL' if same else 'DIFFERENT'} ({what}{'' if finite else ', NOT finite'})")
        if not same or not finite:
            differing.append(name)
    ok = not differing
    print(f"{len(a)} entries, {len(differing)} differ ({', '.join(differing) or 'none'}): "
          + ("every entry is torch.equal" if ok else "FAILED"))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, os.path.dirname(HERE))
    results = run()
    print(f"{len(results)} entries with {os.environ.get('YAT_HIP_LIB') or 'the tree library'}", flush=True)
    torch.save(results, args.out)


if __name__ == "__main__":
    main()
