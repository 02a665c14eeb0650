#!/usr/bin/env python3
"""Same-bits check of the three recipes' ``optimize_device`` between two source trees on ONE built library.

    python scripts/recipe_same_bits.py --tree PARENT_TREE --out parent.pt      # a checkout of the parent commit
    python scripts/recipe_same_bits.py --out work.pt                           # this tree
    python scripts/recipe_same_bits.py --compare parent.pt work.pt > profiles/recipe_fold_a_same_bits.txt

(both runs with ``YAT_HIP_LIB`` naming the same libyat_hip.so).  Per case: a tiny model, fixed seeds, six ``optimize_device``
steps alternating between two latent buckets with caption lengths that change every step; the loss and ``flat_grad`` after
every step are saved.  ``--compare`` prints one ``torch.equal`` verdict per case and exits 1 unless all are equal."""
import argparse
import os
import sys

import torch

BF = torch.bfloat16
SHAPES = ((8, 8), (4, 16))
CAPTIONS = ((40, 128), (7, 99), (1, 65), (128, 3), (64, 17), (100, 13))
CAPTIONS_EMPTY = ((40, 128), (7, 99), (0, 65), (128, 3), (64, 0), (100, 13))


def run_case(recipe, model, in_channels, make_embs, generators, gscale):
    g = torch.Generator().manual_seed(9)
    torch.manual_seed(21)
    torch.cuda.manual_seed(21)
    out = []
    for step in range(6):
        h, w = SHAPES[step % 2]
        latents = (torch.randn(2, in_channels, h, w, generator=g) * 0.5).to(BF)
        loss = recipe.optimize_device(latents, make_embs(step, g), generators(step), gscale=gscale)
        torch.cuda.synchronize()
        out.append((loss.detach().cpu().clone(), model.flat_grad.cpu().clone()))
    return out, getattr(model, "plan_replays", 0)


def cases():
    from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
    from yat_amd.recipe import PixArtRecipe, SanaRecipe, SD3Recipe
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    from yat_amd.sd3 import SD3Config, SD3Transformer2DModelHIP
    sana = SanaConfig(num_layers=2, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=2,
                      cross_attention_head_dim=64, cross_attention_dim=128, caption_channels=96, in_channels=8, out_channels=8,
                      sample_size=32)
    pix = PixArtConfig(num_attention_heads=2, attention_head_dim=24, in_channels=4, out_channels=8, num_layers=2,
                       cross_attention_dim=48, sample_size=8, patch_size=2, caption_channels=64)
    sd3 = SD3Config(sample_size=16, patch_size=2, in_channels=8, out_channels=8, num_layers=2, attention_head_dim=64,
                    num_attention_heads=2, joint_attention_dim=96, caption_projection_dim=128, pooled_projection_dim=64,
                    pos_embed_max_size=24, dual_attention_layers=(0,))

    def ragged(width, captions):
        return lambda step, g: [torch.randn(L, width, generator=g).to(BF) for L in captions[step]]

    def pairs(step, g):
        return [(torch.randn(10, sd3.joint_attention_dim, generator=g).to(BF),
                 torch.randn(sd3.pooled_projection_dim, generator=g).to(BF)) for _ in range(2)]

    fresh = lambda step: torch.Generator()                          # what the trainer hands every step (remembered draws)
    seeded = lambda step: torch.Generator().manual_seed(100 + step)
    global_rng = lambda step: None

    def build(kind):
        if kind == "sana":
            m = SanaTransformer2DModelHIP(sana, device="cuda").init_synthetic(4)
            return SanaRecipe(m, pad_to=128, device="cuda"), m, sana.in_channels
        if kind == "pixart":
            m = PixArtTransformer2DModelHIP(pix, device="cuda").init_synthetic(4)
            return PixArtRecipe(m, pad_to=128, device="cuda"), m, pix.in_channels
        m = SD3Transformer2DModelHIP(sd3, device="cuda").init_synthetic(4)
        return SD3Recipe(m, device="cuda"), m, sd3.in_channels

    # name, model kind, YAT_TEXT_PACK, embeddings, generators, gscale
    return build, [
        ("sana packed text, fresh default generators", "sana", "1", ragged(96, CAPTIONS), fresh, 1.0),
        ("sana YAT_TEXT_PACK=0, seeded generators", "sana", "0", ragged(96, CAPTIONS), seeded, 1.0),
        ("sana gscale 0.5", "sana", "1", ragged(96, CAPTIONS), seeded, 0.5),
        ("pixart device noise", "pixart", "1", ragged(64, CAPTIONS), global_rng, 1.0),
        ("pixart CPU generator", "pixart", "1", ragged(64, CAPTIONS), seeded, 1.0),
        ("pixart empty caption", "pixart", "1", ragged(64, CAPTIONS_EMPTY), global_rng, 1.0),
        ("pixart gscale 0.5", "pixart", "1", ragged(64, CAPTIONS), global_rng, 0.5),
        ("sd3.5 device noise", "sd3", "1", pairs, global_rng, 1.0),
        ("sd3.5 CPU generator", "sd3", "1", pairs, seeded, 1.0),
        ("sd3.5 gscale 0.5", "sd3", "1", pairs, global_rng, 0.5),
    ]


def compare(a_path, b_path):
    a, b = torch.load(a_path), torch.load(b_path)
    ok = set(a) == set(b)
    for name in a:
        (sa, ra), (sb, rb) = a[name], b.get(name, ([], -1))
        same = len(sa) == len(sb) and all(torch.equal(la, lb) and torch.equal(ga, gb) for (la, ga), (lb, gb) in zip(sa, sb))
        ok = ok and same and ra == rb
        losses = ", ".join(f"{float(l):.6f}" for l, _ in sa)
        print(f"{name}: {'equal' if same else 'DIFFERENT'} (6 losses + 6 flat_grad of {sa[0][1].numel()} elements; plan replays "
              f"{ra} / {rb}; losses {losses})")
    print("every case torch.equal" if ok else "NOT all equal")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, args.tree)
    build, todo = cases()
    results = {}
    for name, kind, pack, embs, gens, gscale in todo:
        os.environ["YAT_TEXT_PACK"] = pack
        recipe, model, in_channels = build(kind)
        results[name] = run_case(recipe, model, in_channels, embs, gens, gscale)
        print(f"{name}: {results[name][1]} plan replays, last loss {float(results[name][0][-1][0]):.6f}", flush=True)
    torch.save(results, args.out)


if __name__ == "__main__":
    main()
