#!/usr/bin/env python3
"""Same-bits check of the prefill attention kernels, the LPR row norms and the two text encoders between two builds.

    YAT_HIP_LIB=PARENT/yat_amd/libyat_hip.so python scripts/text_fold_same_bits.py --tree PARENT --out parent.pt
    python scripts/text_fold_same_bits.py --out work.pt                                           # this tree, its own library
    python scripts/text_fold_same_bits.py --compare parent.pt work.pt > profiles/textenc_fold_a_same_bits.txt

``YAT_HIP_LIB`` selects the library, ``--tree`` the checkout whose ``yat_amd`` package drives it (default: this one).  On
seeded inputs the outputs of ``t5_attn_fwd``, ``gemma_attn_fwd``, ``vae_attn_fwd``, ``gemma_rmsnorm``, ``t5_rmsnorm``,
``dcae_rmsnorm_bias`` and of both tiny encoders of the GPU tests are saved.  ``--compare`` prints one ``torch.equal`` verdict per
case and exits 1 unless all are equal."""
import argparse
import os
import sys

import torch

BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
LENS = ([1], [65], [1, 65, 300, 17])
NORM_D = (384, 256, 4096, 40)                  # lpr 16, 32, 64, 1
NORM_M = (3, 301)


def randn(*shape, seed, gain=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * gain).to(BF).cuda()


def offsets(lens):
    return torch.tensor([0] + lens).cumsum(0).to(torch.int32).cuda()


def run():
    from yat_amd import ops
    from yat_amd.gemma2 import Gemma2EncoderHIP
    from yat_amd.t5 import T5EncoderHIP, relative_bias_table
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import gemma2_ref
    import t5_ref
    out = {}

    H = 3
    for lens in LENS:
        rows, max_len = sum(lens), max(lens)
        qkv = randn(rows, 3 * H * 64, seed=rows)
        qkv[:, :2 * H * 64] = (qkv[:, :2 * H * 64].float() * 2.5).to(BF)          # logits past +-100, as tests/test_t5_gpu.py
        table = relative_bias_table(randn(32, H, seed=7, gain=3.0), 32, 128, max_len)
        y = torch.full((rows, H * 64), 3.0, dtype=BF, device="cuda")
        out[f"t5_attn_fwd lens {lens} H {H}"] = ops.t5_attn_fwd(qkv, offsets(lens), len(lens), H, 64, max_len, table, y)

    for Hq, Hkv in ((8, 4), (2, 1), (8, 1), (4, 4), (4, 1)):
        for lens in LENS:
            rows = sum(lens)
            qkv = randn(rows, (Hq + 2 * Hkv) * 256, seed=rows + Hq)
            qkv[:, :(Hq + Hkv) * 256] = (qkv[:, :(Hq + Hkv) * 256].float() * 6.0).to(BF)
            for cap in (50.0, 0.0):
                y = torch.full((rows, Hq * 256), 3.0, dtype=BF, device="cuda")
                out[f"gemma_attn_fwd lens {lens} heads {Hq}/{Hkv} cap {cap:g}"] = ops.gemma_attn_fwd(
                    qkv, offsets(lens), len(lens), Hq, Hkv, 256, max(lens), 256 ** -0.5, cap, y)

    B, N = 2, 1008
    for dh in (64, 512):
        qkv = randn(B * N, 3 * dh, seed=dh, gain=2.0)
        y = torch.full((B * N, dh), 3.0, dtype=BF, device="cuda")
        out[f"vae_attn_fwd dh {dh} N {N} B {B}"] = ops.vae_attn_fwd(qkv[:, :dh], qkv[:, dh:2 * dh], qkv[:, 2 * dh:], y, B, N, dh,
                                                                    3 * dh)

    for D in NORM_D:
        for M in NORM_M:
            x, res = randn(M, D, seed=D + M, gain=3.0), randn(M, D, seed=D + M + 1)
            w, b = randn(D, seed=D, gain=0.5), randn(D, seed=D + 1)
            new = lambda: torch.full((M, D), 3.0, dtype=BF, device="cuda")
            tag = f"D {D} M {M}"
            out[f"gemma_rmsnorm {tag}"] = ops.gemma_rmsnorm(x, w, new(), 1e-6)
            out[f"gemma_rmsnorm {tag} residual"] = ops.gemma_rmsnorm(x, w, new(), 1e-6, residual=res)
            h = res.clone()
            out[f"gemma_rmsnorm {tag} residual in place"] = ops.gemma_rmsnorm(x, w, h, 1e-6, residual=h)
            out[f"t5_rmsnorm {tag}"] = ops.t5_rmsnorm(x, w, new(), 1e-6)
            h = res.clone()
            out[f"t5_rmsnorm {tag} residual: y"] = ops.t5_rmsnorm(x, w, new(), 1e-6, residual=h)
            out[f"t5_rmsnorm {tag} residual: sum in place"] = h
            s = new()
            out[f"t5_rmsnorm {tag} residual, sum_out: y"] = ops.t5_rmsnorm(x, w, new(), 1e-6, residual=res, sum_out=s)
            out[f"t5_rmsnorm {tag} residual, sum_out: sum"] = s
            out[f"dcae_rmsnorm_bias {tag}"] = ops.dcae_rmsnorm_bias(x, w, None, new(), 1e-5)
            out[f"dcae_rmsnorm_bias {tag} residual"] = ops.dcae_rmsnorm_bias(x, w, None, new(), 1e-5, residual=res)
            out[f"dcae_rmsnorm_bias {tag} bias + relu"] = ops.dcae_rmsnorm_bias(x, w, b, new(), 1e-5, relu=True)
            out[f"dcae_rmsnorm_bias {tag} bias + residual + relu"] = ops.dcae_rmsnorm_bias(x, w, b, new(), 1e-5, residual=res,
                                                                                           relu=True)

    for name, ref, cls, gain in (("gemma2", gemma2_ref, Gemma2EncoderHIP, 6.0), ("t5", t5_ref, T5EncoderHIP, 2.0)):
        cfg = ref.tiny_config()
        sd = {k: v.to(BF) for k, v in ref.random_state_dict(cfg, seed=3, logit_gain=gain).items()}
        enc = cls(cfg, sd, "cuda")
        g = torch.Generator().manual_seed(5)
        prompts = [torch.randint(1, cfg["vocab_size"], (n,), generator=g) for n in (23, 65)]
        for i, e in enumerate(enc.encode(prompts)):
            out[f"tiny {name} encoder, prompt of {prompts[i].numel()}"] = e
        for i, e in enumerate(enc.encode(list(reversed(prompts)), max_batch=1)):
            out[f"tiny {name} encoder, one prompt per call, prompt of {prompts[1 - i].numel()}"] = e
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in out.items()}


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    ok = set(a) == set(b)
    for name in a:
        same = name in b and a[name].shape == b[name].shape and torch.equal(a[name], b[name])
        finite = bool(torch.isfinite(a[name].float()).all())
        ok = ok and same and finite
        print(f"{name}: {'EQUAL' if same else 'DIFFERENT'} ({a[name].numel()} elements{'' if finite else ', NOT finite'}, "
              f"mean |x| {float(a[name].float().abs().mean()):.4f})")
    print(f"{len(a)} cases: every case torch.equal" if ok else "NOT all equal")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, args.tree)
    results = run()
    print(f"{len(results)} cases with {os.environ.get('YAT_HIP_LIB') or 'the tree library'}", flush=True)
    torch.save(results, args.out)


if __name__ == "__main__":
    main()
