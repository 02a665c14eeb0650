"""Plain LoRA at ranks 17..128 (padded rank R = 32, 64, 128) on the HIP path -- GPU: the matrix-core forms of the three rank-R
kernels against fp64, the paired forward at a slot of max(64, R) columns, one training step against the oracle's restatement of
the peft wrap with the bars of tests/test_lora_gpu.py, and the trainer's YAML path."""
import copy
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
TARGETS = ["conv_inverted", "conv_point", "to_q", "to_k", "to_v", "to_out.0", "linear_1", "linear_2", "proj"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


@pytest.mark.parametrize("rows,R,N,ld", [(77, 32, 520, 520), (1000, 64, 2240, 2240), (333, 128, 1128, 1128), (4096, 32, 64, 192),
                                         (5, 64, 8, 16)])
def test_rank_expand_mfma(rows, R, N, ld):
    """io = bf16(bf16(h w) * scale) and io = bf16(bf16(h w) + io) with the sum on the matrix cores, against the fp64 product
    rounded the same way with the checker of test_rank_expand: its fp32-versus-fp64 term 1e-5 * mag covers a K-term fp32 sum
    (K * 2^-24 = 7.6e-6 at K = 128).  Columns N..ld keep their bits."""
    from yat_amd import ops
    g = torch.Generator().manual_seed(rows + N)
    h, w = (torch.randn(rows, R, generator=g) * 0.3).to(BF).to(DEV), (torch.randn(R, N, generator=g) * 0.2).to(BF).to(DEV)
    buf = torch.randn(rows, ld, generator=g).to(BF).to(DEV)
    prod = (h.double() @ w.double())
    mag = (h.double().abs() @ w.double().abs()).float()
    out = buf.clone()
    ops.rank_expand(h, w, out[:, :N], scale=0.75)
    want = (prod.float().to(BF).float() * 0.75).to(BF)
    err = (out[:, :N].float() - want.float()).abs()
    print(f"[parity] rank_expand R={R} N={N} scaled: max err / bound = {(err / (2.0 ** -6 * want.float().abs() + 1e-5 * mag)).max().item():.3f}")
    ok = err <= 2.0 ** -6 * want.float().abs() + 1e-5 * mag
    assert ok.all() and torch.equal(out[:, N:], buf[:, N:])
    out = buf.clone()
    ops.rank_expand(h, w, out[:, :N], residual=True)
    want = (prod.float().to(BF).float() + buf[:, :N].float()).to(BF)
    err = (out[:, :N].float() - want.float()).abs()
    bound = 2.0 ** -7 * want.float().abs() + 2.0 ** -7 * prod.abs().float() + 1e-5 * mag
    print(f"[parity] rank_expand R={R} N={N} residual: max err / bound = {(err / bound).max().item():.3f}")
    assert (err <= bound).all() and torch.equal(out[:, N:], buf[:, N:])


@pytest.mark.parametrize("rows,R,N,r_out,acc", [(1000, 32, 56, 32, False), (2049, 64, 328, 48, True), (777, 128, 128, 128, False),
                                                (3000, 32, 2240, 24, False), (5000, 128, 8, 100, True),
                                                (32768, 64, 136, 64, True)])       # the last: more chunks than workgroups
def test_small_wgrad_mfma(rows, R, N, r_out, acc):
    """out[q, n] (+)= bf16(sum_row a[row, q] x[row, n]) with the accumulator block split over the waves: one bf16 rounding of the
    result against fp64 (3e-3, the bar of test_lokr_small_wgrad), equal bits on a second call."""
    from yat_amd import ops
    g = torch.Generator().manual_seed(rows + N)
    a, x = (torch.randn(rows, R, generator=g) * 0.1).to(BF).to(DEV), torch.randn(rows, N, generator=g).to(BF).to(DEV)
    out0 = (torch.randn(r_out, N, generator=g) * 0.5).to(BF).to(DEV)
    out = out0.clone()
    ws = torch.empty(int(ops._lib().yat_lokr_small_wgrad_workspace_bytes(rows, R, N)), dtype=torch.uint8, device=DEV)
    ops.lokr_small_wgrad(a, x, out, ws, accumulate=acc)
    want = (a.double().T @ x.double())[:r_out]
    if acc:
        want = want.float().to(BF).double() + out0.double()
    e = rel(out, want)
    print(f"[parity] small_wgrad rows={rows} R={R} N={N}: rel={e:.3e}")
    assert e <= 3e-3
    out2 = out0.clone()
    ops.lokr_small_wgrad(a, x, out2, ws, accumulate=acc)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("R", [32, 128])
def test_small_wgrad_mfma_column_blocks(R):
    """x and out as column blocks of wider NaN-filled matrices (ldx > N, ldo > N): finite result, the NaNs stay where they were."""
    from yat_amd import ops
    rows, N, r_out, c0 = 1500, 200, R - 3, 16
    g = torch.Generator().manual_seed(R)
    a = (torch.randn(rows, R, generator=g) * 0.1).to(BF).to(DEV)
    xw = torch.full((rows, N + 64), float("nan"), dtype=BF, device=DEV)
    ow = torch.full((r_out + 2, N + 40), float("nan"), dtype=BF, device=DEV)
    x = xw[:, c0:c0 + N]
    x.copy_(torch.randn(rows, N, generator=g).to(BF))
    out = ow[:r_out, 8:8 + N]
    ops.lokr_small_wgrad(a, x, out, scale=0.5)
    assert torch.isfinite(out.float()).all()
    assert rel(out, (a.double().T @ x.double())[:r_out] * 0.5) <= 3e-3
    outside = torch.ones_like(ow, dtype=torch.bool)
    outside[:r_out, 8:8 + N] = False
    assert torch.isnan(ow[outside]).all()
    outside = torch.ones_like(xw, dtype=torch.bool)
    outside[:, c0:c0 + N] = False
    assert torch.isnan(xw[outside]).all()


@pytest.mark.parametrize("r", [32, 48, 128])
def test_scatter_b_and_forward_pair(r):
    """test_lora_scatter_b_and_forward_pair's construction at D = 640, M = 520 above rank 16: the shadow holds bf16(scale * B)
    in the first R columns of each target's rows and zeros elsewhere; the paired forward (slot = max(64, R) columns per
    adapter) against pre_add and fp32 under that test's conditions; bit-equal weight gradients."""
    from types import SimpleNamespace
    from yat_amd.lora import LoRAAdapters
    from yat_amd.lokr import adapted_linear
    D, M = 640, 520
    names = ["blk.to_q", "blk.to_k", "blk.to_v", "blk.to_out.0"]
    g = torch.Generator().manual_seed(21)

    def make(pair):
        flat = (torch.randn(4 * D * D, generator=torch.Generator().manual_seed(5)) * D ** -0.5).to(BF).to(DEV)
        model = SimpleNamespace(P={n + ".weight": flat[i * D * D:(i + 1) * D * D].view(D, D) for i, n in enumerate(names)},
                                flat_param=flat, flat_grad=torch.zeros_like(flat))
        ad = LoRAAdapters(model, ["to_q", "to_k", "to_v", "to_out.0"], r=r, alpha=2.0 * r, pair=pair)
        assert ad.pair == pair and ad.scale == 2.0
        return model, ad
    (m1, a1), (m2, a2) = make(True), make(False)
    R = a1.R
    assert R == {32: 32, 48: 64, 128: 128}[r] and a1.slot == max(64, R)
    for e in a1.entries:
        _, bt = a1._views(e, a1.flat_param)
        bt[:r].copy_((torch.randn(r, D, generator=g) * 0.1).to(BF))
    a2.flat_param.copy_(a1.flat_param)
    a1.materialize(True); a2.materialize(True)
    shadow = a1._flatB.view(4, D, D)
    for i, e in enumerate(a1.entries):
        _, bt = a1._views(e, a1.flat_param)
        assert torch.equal(shadow[i, :, :R], (bt.float().T * 2.0).to(BF)) and (shadow[i, :, R:] == 0).all()
        assert (shadow[i, :, r:R] == 0).all()
    x, bias = torch.randn(M, D, generator=g).to(BF).to(DEV), torch.randn(3 * D, generator=g).to(BF).to(DEV)

    def truth(lo, hi):
        W = m1.flat_param[lo * D * D:hi * D * D].view((hi - lo) * D, D).float()
        dW = torch.zeros_like(W)
        for j, e in enumerate(a1.entries[lo:hi]):
            a, bt = (t.float() for t in a1._views(e, a1.flat_param))
            dW[j * D:(j + 1) * D] = (bt.T @ a) * a1.scale
        return x.float() @ (W + dW).T

    def rel32(a, b):
        return ((a.float() - b.float()).norm() / b.float().norm()).item()
    y1 = adapted_linear(a1, x, m1.flat_param[:3 * D * D].view(3 * D, D), bias)
    y2 = adapted_linear(a2, x, m2.flat_param[:3 * D * D].view(3 * D, D), bias)
    t = truth(0, 3) + bias.float()
    print(f"[parity] lora r={r} q|k|v paired={rel32(y1, t):.3e} pre_add={rel32(y2, t):.3e}")
    assert rel32(y1, t) <= rel32(y2, t) * 1.05 + 1e-4 and rel32(y1, t) < 4e-3, (rel32(y1, t), rel32(y2, t))
    o1 = adapted_linear(a1, x, m1.P["blk.to_out.0.weight"])
    o2 = adapted_linear(a2, x, m2.P["blk.to_out.0.weight"])
    t = truth(3, 4)
    print(f"[parity] lora r={r} to_out paired={rel32(o1, t):.3e} pre_add={rel32(o2, t):.3e}")
    assert rel32(o1, t) <= rel32(o2, t) * 1.05 + 1e-4 and rel32(o1, t) < 4e-3
    dy = torch.randn(M, 3 * D, generator=g).to(BF).to(DEV)
    for m, ad in ((m1, a1), (m2, a2)):
        ad.wgrad(dy, x, m.flat_grad[:3 * D * D].view(3 * D, D))
    torch.cuda.synchronize()
    assert torch.equal(a1.flat_grad, a2.flat_grad) and a1.flat_grad.abs().max().item() > 0


@pytest.mark.parametrize("r,alpha", [(32, 64.0), (48, 48.0), (128, 64.0)])
def test_lora_training_step_matches_oracle_above_rank_16(r, alpha, tmp_path):
    """test_lora_training_step_matches_oracle at R = 32, 64, 128 (power-of-two scalings 2, 1, 1/2), lora_B drawn with std
    0.05 * sqrt(8 / r) so the adapter term stays at the size of the rank-8 case; the same assertions and bars."""
    from oracle.sana_ref import SanaConfig as RefCfg, SanaTransformerRef, init_like_pretrained
    from oracle.recipe_ref import FlowMatchSchedule as RefSched, optimize_ref
    from oracle.lora_ref import apply_lora, LoRAWrapped
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    from yat_amd.recipe import SanaRecipe
    from yat_amd.lora import LoRAAdapters
    from yat_amd.optim import FlatAdamW
    # D = 128, so that a rank of 128 is no wider than the layers (the cross-attention width has to follow the model width)
    rcfg = RefCfg.tiny(num_layers=2, num_attention_heads=4, num_cross_attention_heads=4, cross_attention_dim=128)
    ref = SanaTransformerRef(rcfg)
    init_like_pretrained(ref, 0)
    ref_bf = copy.deepcopy(ref).to(BF)
    kw = {k: getattr(rcfg, k) for k in SanaConfig.__dataclass_fields__}
    hip = SanaTransformer2DModelHIP(SanaConfig(**kw), device=DEV)
    hip.load_state_dict(ref_bf.state_dict())
    ad = LoRAAdapters(hip, TARGETS, r=r, alpha=alpha)
    assert ad.R == {32: 32, 48: 64, 128: 128}[r]
    g = torch.Generator().manual_seed(11)
    for e in ad.entries:
        _, bt = ad._views(e, ad.flat_param)
        bt[:r].copy_((torch.randn(r, e["out"], generator=g) * 0.05 * (8.0 / r) ** 0.5).to(BF))
    wrapped = apply_lora(ref_bf, TARGETS, r=r, alpha=alpha)
    assert sorted(wrapped) == sorted(e["module"] for e in ad.entries)
    sd = ad.state_dict()
    for name, w in wrapped.items():
        pre = f"base_model.model.{name}."
        with torch.no_grad():
            w.lora_A.copy_(sd[pre + "lora_A.weight"].cpu())
            w.lora_B.copy_(sd[pre + "lora_B.weight"].cpu())
    ref_32 = copy.deepcopy(ref_bf).float()
    B, h, w_ = 2, 6, 10
    latents = (torch.randn(B, rcfg.in_channels, h, w_, generator=g) * 0.5).to(BF)
    embs = [torch.randn(L, rcfg.caption_channels, generator=g).to(BF) for L in (9, 30)]
    outs = {}
    for tag, model, dt in (("bf16", ref_bf, BF), ("fp32", ref_32, torch.float32)):
        model.train()
        loss, pred, _ = optimize_ref(model, RefSched(), latents, embs, torch.Generator().manual_seed(3), pad_to=32, dtype=dt)
        loss.backward()
        outs[tag] = (loss.detach(), pred.detach(), {n: (m.lora_A.grad, m.lora_B.grad) for n, m in model.named_modules()
                                                   if isinstance(m, LoRAWrapped)})
    recipe = SanaRecipe(hip, pad_to=32, device=DEV)
    hip.train()
    loss, pred, _ = recipe.optimize(latents, embs, torch.Generator().manual_seed(3), return_pred=True)
    loss.backward()
    torch.cuda.synchronize()
    l32, lbf, lh = float(outs["fp32"][0]), float(outs["bf16"][0]), float(loss.detach())
    print(f"[parity] lora r={r} loss hip={lh:.6f} oracle_bf16={lbf:.6f} fp32={l32:.6f}")
    assert abs(lh - l32) <= 1.15 * abs(lbf - l32) + 2e-3 * abs(l32)
    e_h, e_r = rel(pred, outs["fp32"][1]), rel(outs["bf16"][1], outs["fp32"][1])
    print(f"[parity] lora r={r} pred hip_vs_fp32={e_h:.3e} oracle_bf16_vs_fp32={e_r:.3e}")
    assert e_h <= 1.15 * e_r + 1e-3
    hip_g, bf_g, f_g = [], [], []
    for e in ad.entries:
        ga, gbt = ad._views(e, ad.flat_grad)
        assert ga[r:].abs().sum().item() == 0 and gbt[r:].abs().sum().item() == 0          # rank padding stays untouched
        hip_g += [ga[:r].float().flatten().cpu(), gbt[:r].t().float().flatten().cpu()]
        bf_g += [t.float().flatten() for t in outs["bf16"][2][e["module"]]]
        f_g += [t.float().flatten() for t in outs["fp32"][2][e["module"]]]
    hg, bg, fg = torch.cat(hip_g), torch.cat(bf_g), torch.cat(f_g)
    e_h, e_r = rel(hg, fg), rel(bg, fg)
    print(f"[parity] lora r={r} adapter grads hip_vs_fp32={e_h:.3e} oracle_bf16_vs_fp32={e_r:.3e} (n={hg.numel()})")
    assert torch.isfinite(hg).all() and fg.abs().max() > 0
    assert e_h <= 1.15 * e_r + 2e-3
    for e in ad.entries:                                    # padding rows of the parameters: zero before the step ...
        a, bt = ad._views(e, ad.flat_param)
        assert a[r:].abs().sum().item() == 0 and bt[r:].abs().sum().item() == 0
    before = hip.flat_param.clone()
    opt = FlatAdamW(ad, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
    p0 = ad.flat_param.clone()
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(before, hip.flat_param) and not torch.equal(p0, ad.flat_param)
    for e in ad.entries:                                    # ... and after it
        a, bt = ad._views(e, ad.flat_param)
        assert a[r:].abs().sum().item() == 0 and bt[r:].abs().sum().item() == 0
    ad.save_pretrained(str(tmp_path / "a"))
    from safetensors.torch import load_file
    saved = load_file(str(tmp_path / "a" / "adapter_model.safetensors"))
    again = LoRAAdapters(hip, TARGETS, r=r, alpha=alpha)
    again.load_state_dict(saved)
    assert torch.equal(again.flat_param, ad.flat_param)
    k0 = f"base_model.model.{ad.entries[0]['module']}."
    assert saved[k0 + "lora_A.weight"].shape == (r, ad.entries[0]["inn"]) and saved[k0 + "lora_B.weight"].shape == (ad.entries[0]["out"], r)


def _write_shards(tmp, cfg, n_shards=2, per=16):
    from yat_amd.common.shards import write_shard
    from yat_amd.common.aspect_ratios import ASPECT_RATIO_1024_BIN
    g = torch.Generator().manual_seed(0)
    paths = []
    for s in range(n_shards):
        samples = []
        for i in range(per):
            ratio = ["1.0", "0.5", "2.0"][(i + s) % 3]
            H, W = ASPECT_RATIO_1024_BIN[ratio]
            L = int(torch.randint(3, 40, (1,), generator=g))
            samples.append(dict(__key__=f"{s:03d}{i:05d}", ratio=ratio,
                                latent=(torch.randn(cfg.in_channels, int(H) // 128, int(W) // 128, generator=g) * 0.5).to(BF),
                                emb=torch.randn(L, cfg.caption_channels, generator=g).to(BF)))
        p = str(tmp / f"shard-{s:06d}.tar")
        write_shard(p, samples)
        paths.append(p)
    return paths


def test_trainer_lora_rank_32(tmp_path, monkeypatch):
    """``lora_rank: 32`` through the trainer's YAML keys on a tiny model: initialize() builds LoRAAdapters with R = 32, two
    steps train only the adapters, and a second trainer reloads the saved adapter through ``lora_pretrained``."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from safetensors.torch import load_file
    from train_sana import SanaModel
    from yat_amd.common.training_parameters_reader import TrainingParameters
    from yat_amd.lora import LoRAAdapters
    from yat_amd.sana import SanaConfig
    cfg = SanaConfig(num_layers=2, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=2,
                     cross_attention_head_dim=64, cross_attention_dim=128, caption_channels=96, in_channels=8, out_channels=8,
                     sample_size=32)
    paths = _write_shards(tmp_path, cfg)
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", *[f"  - {p}" for p in paths], "num_shards: 2", "dataset_seed: 7",
        "batch_size: 4", "learning_rate: 1e-3", "steps: 2", "num_steps_per_validation: 2", "validation_prompts:", "  - x",
        "bfloat16: true", "lora_rank: 32", "lora_alpha: 32", "lora_algo: lora",
        "lora_target_modules:", *[f"  - {t}" for t in TARGETS], "aspect_ratio: 1024", ""]))
    monkeypatch.chdir(tmp_path)
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    trainer = SanaModel(params, config=cfg)
    trainer.initialize()
    assert type(trainer.adapters) is LoRAAdapters and (trainer.adapters.r, trainer.adapters.R) == (32, 32)
    base = trainer.model.flat_param.clone()
    trainer.run()
    torch.cuda.synchronize()
    assert type(trainer.adapters) is LoRAAdapters and trainer.adapters.R == 32 and len(trainer.loss_history) == 2
    assert all(torch.isfinite(torch.tensor([float(l) for l in trainer.loss_history])))
    assert torch.equal(base, trainer.model.flat_param), "the frozen base moved"
    ck = tmp_path / "models" / sorted(os.listdir(tmp_path / "models"))[-1]
    sd = load_file(str(ck / "adapter_model.safetensors"))
    assert json.loads((ck / "adapter_config.json").read_text())["r"] == 32
    assert sd["base_model.model.transformer_blocks.1.attn2.to_out.0.lora_B.weight"].shape == (128, 32)
    assert any(v.abs().max() > 0 for k, v in sd.items() if k.endswith("lora_B.weight")), "lora_B never left its zero init"
    yaml_path.write_text(yaml_path.read_text() + f"lora_pretrained: {ck}\n")
    params2 = TrainingParameters()
    params2.read_yaml(str(yaml_path))
    resumed = SanaModel(params2, config=cfg)
    resumed.initialize()
    assert type(resumed.adapters) is LoRAAdapters and resumed.adapters.R == 32
    for k, v in resumed.adapters.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
