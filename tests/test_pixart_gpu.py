"""PixArt-Sigma path (BASELINE config 3) on the GPU vs the CPU oracle (oracle/pixart_ref.py, parity unpinned: the
diffusers sub-modules are restated from recall; the recipe follows train_pixart_sigma.py:151-185 line by line).

Tolerances: the glue kernels (patch gather/scatter, position table add, add_noise, bf16 MSE) are checked BIT-EXACT against
torch on the CPU; the end-to-end step uses the same yardstick as the SANA tests -- as close to the fp32 truth as the
reference's own bf16 arithmetic: rel_l2(hip, fp32) <= 1.15 * rel_l2(oracle_bf16, fp32) + 1e-3.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


# ---------------------------------------------------------------------------------------------- glue kernels
@pytest.mark.parametrize("B,C,H,W,p", [(2, 4, 8, 12, 2), (1, 8, 6, 6, 1), (3, 4, 16, 8, 4)])
def test_patch_rearrange_matches_torch(B, C, H, W, p):
    from yat_amd import ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, H, W, generator=g).to(BF)
    h, w = H // p, W // p
    # channel-major: the im2col rows of Conv2d(k=p, s=p); F.unfold yields exactly that column order
    want = torch.nn.functional.unfold(x.float(), kernel_size=p, stride=p).transpose(1, 2).reshape(B * h * w, C * p * p).to(BF)
    got = ops.patch_rearrange(x.to(DEV), torch.empty(B * h * w, C * p * p, dtype=BF, device=DEV), B, C, H, W, p, True, True)
    assert torch.equal(got.cpu(), want)
    # "nhwpqc->nchpwq" scatter (unpatchify) and its gather (the backward)
    tok = torch.randn(B * h * w, p * p * C, generator=g).to(BF)
    want_img = torch.einsum("nhwpqc->nchpwq", tok.reshape(B, h, w, p, p, C)).reshape(B, C, H, W)
    img = ops.patch_rearrange(tok.to(DEV), torch.empty(B, C, H, W, dtype=BF, device=DEV), B, C, H, W, p, False, False)
    assert torch.equal(img.cpu(), want_img)
    back = ops.patch_rearrange(img, torch.empty_like(tok, device=DEV), B, C, H, W, p, False, True)
    assert torch.equal(back.cpu(), tok)


def test_pos_embed_table_and_add():
    from oracle.pixart_ref import sincos_2d
    from yat_amd.pixart import sincos_pos_embed
    from yat_amd import ops
    for (D, h, w, base, interp) in [(48, 4, 4, 4, 1), (1152, 6, 10, 64, 2), (64, 16, 8, 8, 2)]:
        a, b = sincos_pos_embed(D, h, w, base, interp), sincos_2d(D, h, w, base, interp)
        assert torch.equal(a, b), (D, h, w)
    pos = sincos_2d(64, 3, 5, 4, 1)
    x = torch.randn(2 * 15, 64, generator=torch.Generator().manual_seed(1)).to(BF)
    want = (x.view(2, 15, 64) + pos[None]).to(BF).view(30, 64)          # bf16 + fp32 -> fp32 sum -> bf16
    got = ops.add_pos_embed(x.to(DEV), pos.to(DEV))
    assert torch.equal(got.cpu(), want)


def test_ddpm_add_noise_bit_exact():
    from oracle.pixart_ref import DDPMSchedule as Ref
    from yat_amd.scheduler import DDPMSchedule
    from yat_amd import ops
    ref, sch = Ref(), DDPMSchedule()
    assert torch.equal(ref.timesteps, sch.timesteps) and torch.equal(ref.alphas_cumprod, sch.alphas_cumprod)
    assert sch.timesteps[0] == 999 and sch.timesteps[-1] == 0
    g = torch.Generator().manual_seed(2)
    x, n = torch.randn(5, 4, 8, 6, generator=g).to(BF), torch.randn(5, 4, 8, 6, generator=g).to(BF)
    t = torch.tensor([0, 999, 500, 37, 801])
    want = ref.add_noise(x, n, t)
    got = ops.ddpm_add_noise(x.to(DEV), n.to(DEV), sch.sqrt_alpha_prod[t].to(DEV), sch.sqrt_one_minus_alpha_prod[t].to(DEV))
    assert want.dtype == BF and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("shape", [(2, 4, 16, 16), (3, 4, 24, 20), (8, 4, 128, 128)])
def test_mse_bf16_chunk_matches_torch(shape):
    """loss and gradient of MSELoss()(out.chunk(2, 1)[0], noise) in bf16, against torch's CPU bf16 kernels."""
    from yat_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(3)
    out = torch.randn(B, 2 * C, H, W, generator=g).to(BF).requires_grad_(True)
    noise = torch.randn(B, C, H, W, generator=g).to(BF)
    loss = torch.nn.MSELoss()(out.chunk(2, 1)[0].to(BF), noise)
    loss.backward()
    l = torch.zeros(1, dtype=torch.float32, device=DEV)
    d = torch.full(out.shape, 7.0, dtype=BF, device=DEV)
    ops.mse_bf16_chunk(out.detach().to(DEV), noise.to(DEV), l, d, torch.empty(256, dtype=torch.float32, device=DEV))
    assert loss.dtype == BF
    # the mean's summation order differs (fp32 partial sums): allow one bf16 ulp on the loss, none on the gradient
    assert abs(l.item() - loss.item()) <= 2.0 ** -7 * abs(loss.item()), (l.item(), loss.item())
    assert torch.equal(d.cpu(), out.grad)
    assert (d[:, C:] == 0).all()


# ---------------------------------------------------------------------------------------------- end to end
def _setup(cfg_kw, B, Hl, Wl, lens, seed=0):
    from oracle.pixart_ref import PixArtConfig as RefCfg, PixArtTransformerRef, init_like_pretrained
    from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
    rcfg = RefCfg.tiny(**cfg_kw)
    ref = PixArtTransformerRef(rcfg)
    init_like_pretrained(ref, seed)
    ref_bf = copy.deepcopy(ref).to(BF)               # also rounds the pos_embed buffer, as pipe.transformer.to(bf16) does
    ref_32 = copy.deepcopy(ref_bf).float()
    kw = {k: getattr(rcfg, k) for k in PixArtConfig.__dataclass_fields__}
    hip = PixArtTransformer2DModelHIP(PixArtConfig(**kw), device=DEV)
    hip.load_state_dict(ref_bf.state_dict())
    g = torch.Generator().manual_seed(100 + seed)
    latents = (torch.randn(B, rcfg.in_channels, Hl, Wl, generator=g) * 0.5).to(BF)
    embs = [torch.randn(L, rcfg.caption_channels, generator=g).to(BF) for L in lens]
    noise = torch.randn(B, rcfg.in_channels, Hl, Wl, generator=g).to(BF)
    return ref_bf, ref_32, hip, latents, embs, noise


@pytest.mark.parametrize("B,Hl,Wl,lens,pad_to,layers", [
    (2, 8, 8, [5, 16], 16, 2),               # the square base grid (bf16-rounded position buffer)
    (3, 12, 20, [7, 40, 1], 64, 2),          # another aspect bucket: table recomputed in fp32
    (2, 32, 16, [100, 33], 300, 3),
])
def test_step_matches_oracle(B, Hl, Wl, lens, pad_to, layers):
    from oracle.pixart_ref import DDPMSchedule as RefSched, pixart_optimize_ref
    from yat_amd.recipe import PixArtRecipe
    from yat_amd.optim import FlatAdamW
    ref_bf, ref_32, hip, latents, embs, noise = _setup(dict(num_layers=layers), B, Hl, Wl, lens)
    sched = RefSched()
    # identical draws on all three: the noise tensor is passed in, the timestep draw comes from equal fresh CPU generators
    loss_bf, out_bf, _, ts = pixart_optimize_ref(ref_bf, sched, latents, embs, noise, torch.Generator(), pad_to, True)
    loss_32, out_32, _, _ = pixart_optimize_ref(ref_32, sched, latents.float(), [e.float() for e in embs], noise.float(),
                                                torch.Generator(), pad_to, True)
    loss_bf.backward()
    loss_32.backward()
    recipe = PixArtRecipe(hip, pad_to=pad_to, device=DEV)
    loss, out, _ = recipe.optimize(latents, embs, torch.Generator(), return_pred=True, noise=noise.to(DEV))
    loss.backward()
    torch.cuda.synchronize()

    assert loss.dtype == BF and out.shape == (B, 2 * latents.shape[1], Hl, Wl)
    l_h, l_b, l_t = loss.item(), loss_bf.item(), loss_32.item()
    print(f"[pixart] loss hip={l_h:.6f} oracle_bf16={l_b:.6f} oracle_fp32={l_t:.6f} timesteps={ts.tolist()}")
    assert abs(l_h - l_t) <= 1.15 * abs(l_b - l_t) + 2.0 ** -7 * abs(l_t)      # the loss itself is a bf16 number
    e_h, e_b, e_hb = rel(out, out_32), rel(out_bf, out_32), rel(out, out_bf)
    print(f"[pixart] out   hip_vs_fp32={e_h:.3e} oracle_bf16_vs_fp32={e_b:.3e} hip_vs_oracle_bf16={e_hb:.3e}")
    assert e_h <= 1.15 * e_b + 1e-3

    p32 = dict(ref_32.named_parameters())
    worst, num_h, num_b, den = [], 0.0, 0.0, 0.0
    for name, pb in ref_bf.named_parameters():
        gh, gb, gt = hip.G[name].float().cpu(), pb.grad.float(), p32[name].grad.float()
        assert torch.isfinite(gh).all(), name
        num_h += (gh - gt).pow(2).sum().item()
        num_b += (gb - gt).pow(2).sum().item()
        den += gt.pow(2).sum().item()
        worst.append((rel(gh, gt), rel(gb, gt), name))
    tot_h, tot_b = (num_h / den) ** 0.5, (num_b / den) ** 0.5
    print(f"[pixart] grads (all params) hip_vs_fp32={tot_h:.3e} oracle_bf16_vs_fp32={tot_b:.3e}")
    for eh, eb, name in sorted(worst, reverse=True)[:8]:
        print(f"[pixart]   {name}: hip={eh:.3e} oracle_bf16={eb:.3e}")
    assert tot_h <= 1.15 * tot_b + 1e-3
    for eh, eb, name in worst:
        if name.endswith("to_k.bias"):
            # softmax is invariant to a per-head constant added to every key score: the true gradient is exactly zero and
            # both bf16 paths only hold rounding noise there -- compare magnitudes, not relative errors
            gh, gb = hip.G[name].float().abs().max().item(), dict(ref_bf.named_parameters())[name].grad.float().abs().max().item()
            assert gh <= 4.0 * gb + 1e-6, (name, gh, gb)
            continue
        assert eh <= 2.0 * eb + 2e-2, (name, eh, eb)

    # one clip + AdamW step against torch's CPU optimizer fed with the oracle's bf16 gradients
    opt_ref = torch.optim.AdamW(ref_bf.parameters(), lr=1e-3, weight_decay=0.01)
    total = torch.nn.utils.clip_grad_norm_(ref_bf.parameters(), max_norm=1.0)
    opt_ref.step()
    opt = FlatAdamW(hip, lr=1e-3, weight_decay=0.01)
    opt.step()
    torch.cuda.synchronize()
    assert abs(opt.grad_norm.item() - total.float().item()) <= 2e-2 * total.float().item()
    n_bad = n_all = 0
    for name, pb in ref_bf.named_parameters():
        a, b = hip.P[name].float().cpu(), pb.data.float()
        n_bad += ((a - b).abs() > 2.0 ** -7 * b.abs().clamp_min(1e-30)).sum().item()
        n_all += b.numel()
    print(f"[pixart] AdamW: {n_bad}/{n_all} parameters differ by more than 1 bf16 ulp from torch CPU")
    assert n_bad <= 0.01 * n_all


def test_state_dict_roundtrip(tmp_path):
    from yat_amd.pixart import PixArtTransformer2DModelHIP
    ref_bf, _, hip, latents, embs, _ = _setup(dict(num_layers=1), 1, 8, 8, [3])
    sd = hip.state_dict()
    want = {k: v for k, v in ref_bf.state_dict().items() if k != "pos_embed.pos_embed"}
    assert set(sd) == set(want)
    for k, v in want.items():
        assert torch.equal(sd[k].cpu(), v), k
    hip.save_pretrained(str(tmp_path / "m"))
    from safetensors.torch import load_file
    saved = load_file(str(tmp_path / "m" / "diffusion_pytorch_model.safetensors"))
    assert torch.equal(saved["pos_embed.pos_embed"], ref_bf.state_dict()["pos_embed.pos_embed"])      # the buffer travels too
    again = PixArtTransformer2DModelHIP.from_pretrained(str(tmp_path / "m"), device=DEV)
    assert torch.equal(again.flat_param, hip.flat_param)
    with torch.no_grad():
        enc = torch.zeros(1, 8, ref_bf.cfg.caption_channels, dtype=BF, device=DEV)
        out = hip(latents.to(DEV), encoder_hidden_states=enc, timestep=torch.tensor([500]),
                  encoder_attention_mask=torch.ones(1, 8, dtype=torch.long)).sample
    assert out.shape == (1, 8, 8, 8) and torch.isfinite(out.float()).all()


def test_use_additional_conditions_raises():
    from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
    with pytest.raises(ValueError):
        PixArtTransformer2DModelHIP(PixArtConfig(num_layers=1, use_additional_conditions=True), device=DEV)


def test_overfits_a_fixed_batch():
    """Learning sanity at real width (D=1152, 16 heads x 72, 2 blocks, 32x32 latents = 256 tokens): 40 steps on one fixed
    (batch, noise, timestep) draw must drive the epsilon-prediction loss down."""
    from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
    from yat_amd.recipe import PixArtRecipe
    from yat_amd.optim import FlatAdamW
    cfg = PixArtConfig(num_layers=2, sample_size=32)
    model = PixArtTransformer2DModelHIP(cfg, device=DEV).init_synthetic(seed=0)
    opt = FlatAdamW(model, lr=2e-4, weight_decay=0.0, max_grad_norm=1.0, overlap_update=True)
    recipe = PixArtRecipe(model, device=DEV)
    g = torch.Generator().manual_seed(3)
    latents = (torch.randn(4, 4, 32, 32, generator=g) * 0.5).to(BF)
    embs = [torch.randn(L, cfg.caption_channels, generator=g).to(BF) for L in (30, 120, 64, 300)]
    noise = torch.randn(4, 4, 32, 32, generator=g).to(BF).to(DEV)
    losses = []
    for _ in range(40):
        loss = recipe.optimize(latents, embs, torch.Generator().manual_seed(9), noise=noise)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    model.join_pending_update()
    torch.cuda.synchronize()
    print("[pixart] overfit losses:", [round(x, 4) for x in losses[::5]], round(losses[-1], 4))
    assert all(l == l and l < 1e4 for l in losses)
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])


def test_pixart_lora_step_matches_oracle():
    """LoRA adapters (lora_algo: lora) on the PixArt-Sigma path: the adapter hooks of the model are the same as SANA's.
    One adapted step on the tiny configuration vs the oracle's peft-wrapped model in bf16 and fp32."""
    from oracle.pixart_ref import DDPMSchedule as RefSched, pixart_optimize_ref
    from oracle.lora_ref import apply_lora, LoRAWrapped
    from yat_amd.recipe import PixArtRecipe
    from yat_amd.lora import LoRAAdapters
    targets = ["to_q", "to_k", "to_v", "to_out.0", "linear_1", "linear_2", "proj"]
    ref_bf, _, hip, latents, embs, noise = _setup(dict(num_layers=2), 2, 12, 20, [7, 40])
    r = 4
    ad = LoRAAdapters(hip, targets, r=r, alpha=4.0)
    g = torch.Generator().manual_seed(21)
    for e in ad.entries:
        _, bt = ad._views(e, ad.flat_param)
        bt[:r].copy_((torch.randn(r, e["out"], generator=g) * 0.05).to(BF))
    wrapped = apply_lora(ref_bf, targets, r=r, alpha=4.0)
    assert sorted(wrapped) == sorted(e["module"] for e in ad.entries) and "transformer_blocks.0.ff.net.0.proj" in wrapped
    sd = ad.state_dict()
    for name, w in wrapped.items():
        with torch.no_grad():
            w.lora_A.copy_(sd[f"base_model.model.{name}.lora_A.weight"].cpu())
            w.lora_B.copy_(sd[f"base_model.model.{name}.lora_B.weight"].cpu())
    ref_32 = copy.deepcopy(ref_bf).float()
    outs = {}
    for tag, model, cast in (("bf16", ref_bf, lambda t: t), ("fp32", ref_32, lambda t: t.float())):
        model.train()
        loss, out, _, _ = pixart_optimize_ref(model, RefSched(), cast(latents), [cast(e_) for e_ in embs], cast(noise),
                                              torch.Generator(), 64, True)
        loss.backward()
        outs[tag] = (loss.detach(), out.detach(), {n: (m.lora_A.grad, m.lora_B.grad) for n, m in model.named_modules()
                                                  if isinstance(m, LoRAWrapped)})
    recipe = PixArtRecipe(hip, pad_to=64, device=DEV)
    hip.train()
    base = hip.flat_param.clone()
    loss, out, _ = recipe.optimize(latents, embs, torch.Generator(), return_pred=True, noise=noise.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    e_h, e_r = rel(out, outs["fp32"][1]), rel(outs["bf16"][1], outs["fp32"][1])
    print(f"[pixart] lora out hip_vs_fp32={e_h:.3e} oracle_bf16_vs_fp32={e_r:.3e}")
    assert e_h <= 1.15 * e_r + 1e-3
    hip_g, bf_g, f_g = [], [], []
    for e in ad.entries:
        ga, gbt = ad._views(e, ad.flat_grad)
        hip_g += [ga[:r].float().flatten().cpu(), gbt[:r].t().float().flatten().cpu()]
        bf_g += [t.float().flatten() for t in outs["bf16"][2][e["module"]]]
        f_g += [t.float().flatten() for t in outs["fp32"][2][e["module"]]]
    hg, bg, fg = torch.cat(hip_g), torch.cat(bf_g), torch.cat(f_g)
    e_h, e_r = rel(hg, fg), rel(bg, fg)
    print(f"[pixart] lora adapter grads hip_vs_fp32={e_h:.3e} oracle_bf16_vs_fp32={e_r:.3e} (n={hg.numel()})")
    assert torch.isfinite(hg).all() and fg.abs().max() > 0 and e_h <= 1.15 * e_r + 2e-3
    assert torch.equal(base, hip.flat_param)


def test_real_width_block_matches_oracle():
    """One block at the real width (D = 1152, 16 heads x 72, T5 width 4096, T = 300 padded keys) on 64x64 latents (1024
    tokens, a non-base grid): the head-dim-72 attention instantiations, the K = 1152 / 4608 GEMM shapes and the GELU epilogue
    against the oracle in bf16 and fp32 -- same criterion as the tiny configurations."""
    from oracle.pixart_ref import (PixArtConfig as RefCfg, PixArtTransformerRef, init_like_pretrained,
                                   DDPMSchedule as RefSched, pixart_optimize_ref)
    from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
    from yat_amd.recipe import PixArtRecipe
    rcfg = RefCfg(num_layers=1)
    ref = PixArtTransformerRef(rcfg)
    init_like_pretrained(ref, 3)
    ref_bf = copy.deepcopy(ref).to(BF)
    ref_32 = copy.deepcopy(ref_bf).float()
    hip = PixArtTransformer2DModelHIP(PixArtConfig(num_layers=1), device=DEV)
    hip.load_state_dict(ref_bf.state_dict())
    g = torch.Generator().manual_seed(17)
    latents = (torch.randn(2, 4, 64, 64, generator=g) * 0.5).to(BF)
    embs = [torch.randn(L, rcfg.caption_channels, generator=g).to(BF) for L in (300, 77)]
    noise = torch.randn(2, 4, 64, 64, generator=g).to(BF)
    loss_bf, out_bf, _, _ = pixart_optimize_ref(ref_bf, RefSched(), latents, embs, noise, torch.Generator(), 300, True)
    loss_32, out_32, _, _ = pixart_optimize_ref(ref_32, RefSched(), latents.float(), [e.float() for e in embs], noise.float(),
                                                torch.Generator(), 300, True)
    loss_bf.backward()
    loss_32.backward()
    recipe = PixArtRecipe(hip, pad_to=300, device=DEV)
    loss, out, _ = recipe.optimize(latents, embs, torch.Generator(), return_pred=True, noise=noise.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    l_h, l_b, l_t = loss.item(), loss_bf.item(), loss_32.item()
    e_h, e_b = rel(out, out_32), rel(out_bf, out_32)
    print(f"[pixart] real width: loss hip={l_h:.5f} oracle_bf16={l_b:.5f} fp32={l_t:.5f}; out hip={e_h:.3e} oracle_bf16={e_b:.3e}")
    assert abs(l_h - l_t) <= 1.15 * abs(l_b - l_t) + 2.0 ** -7 * abs(l_t)
    assert e_h <= 1.15 * e_b + 1e-3
    p32 = dict(ref_32.named_parameters())
    num_h = num_b = den = 0.0
    for name, pb in ref_bf.named_parameters():
        gh, gb, gt = hip.G[name].float().cpu(), pb.grad.float(), p32[name].grad.float()
        assert torch.isfinite(gh).all(), name
        num_h += (gh - gt).pow(2).sum().item(); num_b += (gb - gt).pow(2).sum().item(); den += gt.pow(2).sum().item()
    tot_h, tot_b = (num_h / den) ** 0.5, (num_b / den) ** 0.5
    print(f"[pixart] real width: grads hip_vs_fp32={tot_h:.3e} oracle_bf16_vs_fp32={tot_b:.3e}")
    assert tot_h <= 1.15 * tot_b + 1e-3


def test_pixart_launch_plan_replay_is_bit_identical():
    """PixArt-Sigma's device path (``PixArtRecipe.train_step_device`` -> ``forward_device`` / ``backward_device``) replays a
    recorded launch plan once a (bucket shape, buffer addresses, schedule) combination has run (yat_amd/flat.py ``planned``;
    train_pixart_sigma.py:151-185 is the step): eight optimizer steps alternating between two buckets, with new latents,
    captions of other lengths (and hence another attention work list length) and new draws every step, must give
    bit-identical losses and parameters with plans on and off."""
    from yat_amd import ops
    from yat_amd.optim import FlatAdamW
    from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
    from yat_amd.recipe import PixArtRecipe
    cfg = PixArtConfig(num_attention_heads=2, attention_head_dim=24, in_channels=4, out_channels=8, num_layers=3,
                       cross_attention_dim=48, sample_size=8, patch_size=2, caption_channels=64)
    B, T = 4, 128
    runs = []
    for plans in (True, False):
        hip = PixArtTransformer2DModelHIP(cfg, device=DEV).init_synthetic(4)
        hip.use_plans = plans
        opt = FlatAdamW(hip, lr=1e-3, weight_decay=0.01, overlap_update=True)
        recipe = PixArtRecipe(hip, pad_to=T, device=DEV)
        g = torch.Generator().manual_seed(9)
        shapes = ((8, 16), (12, 8))
        lat = [torch.empty(B, cfg.in_channels, h, w, dtype=BF, device=DEV) for h, w in shapes]       # persistent per bucket
        noise = [torch.empty_like(t) for t in lat]
        src = torch.empty(B * T, cfg.caption_channels, dtype=BF, device=DEV)
        offs = torch.empty(B + 1, dtype=torch.int32, device=DEV)
        work = torch.empty(B * ((T + 63) // 64), 2, dtype=torch.int32, device=DEV)
        enc = torch.empty(B, T, cfg.caption_channels, dtype=BF, device=DEV)
        mask = torch.empty(B, T, dtype=torch.int64, device=DEV)
        bias, kvl = torch.empty(B, T, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
        t_dev, a_dev, c_dev = torch.empty(B, device=DEV), torch.empty(B, dtype=BF, device=DEV), torch.empty(B, dtype=BF, device=DEV)
        loss_dev = torch.zeros(1, device=DEV)
        losses = []
        for step in range(8):
            k = step % 2
            lat[k].copy_((torch.randn(lat[k].shape, generator=g) * 0.5).to(BF))
            noise[k].copy_(torch.randn(lat[k].shape, generator=g).to(BF))
            lens = torch.randint(1, T + 1, (B,), generator=g).tolist()
            o = [0]
            for L_ in lens:
                o.append(o[-1] + L_)
            src[:o[-1]].copy_(torch.randn(o[-1], cfg.caption_channels, generator=g).to(BF))
            offs.copy_(torch.tensor(o, dtype=torch.int32))
            wl = ops.kv_work_list(lens, T, "cpu")
            work[:wl.shape[0]].copy_(wl)
            ops.pad_mask(src, offs, B, T, cfg.caption_channels, enc, mask, bias, kvl)
            t, a, c = recipe.scheduler.sample(B, torch.Generator().manual_seed(100 + step))
            t_dev.copy_(t); a_dev.copy_(a); c_dev.copy_(c)
            recipe.train_step_device(lat[k], enc, (bias, kvl), noise[k], t_dev, a_dev, c_dev, loss_dev, kv_work=work[:wl.shape[0]])
            losses.append(loss_dev.clone())
            opt.step()
        hip.join_pending_update()
        torch.cuda.synchronize()
        runs.append((torch.cat(losses).cpu(), hip.flat_param.clone(), getattr(hip, "plan_replays", 0), len(hip._plans)))
    (l_a, p_a, replays, nplans), (l_b, p_b, r_b, n_b) = runs
    print(f"[plans] pixart: {nplans} plans recorded, {replays} replays; losses {l_a.tolist()}")
    assert r_b == 0 and n_b == 0
    assert replays >= 2 * 4 and nplans <= 8
    assert torch.isfinite(l_a).all() and torch.equal(l_a, l_b) and torch.equal(p_a, p_b)


def test_pixart_device_path_equals_autograd_path():
    """``PixArtRecipe.optimize_device`` (what ``PixartSigmaTrainer.optimize`` runs when training: one packed H2D copy, noise
    drawn on the device into a persistent buffer, launch plans) against ``optimize`` + ``loss.backward()`` (the autograd path
    every oracle test pins) on the same host batch and the same global RNG state (train_pixart_sigma.py:170,172 draw from the
    global device / CPU streams): loss and every gradient bit-identical, also on a replayed plan and with a CPU generator;
    ``gscale`` (gradient accumulation, common/trainer.py:317,343) scales the gradient."""
    from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
    from yat_amd.recipe import PixArtRecipe
    cfg = PixArtConfig(num_attention_heads=2, attention_head_dim=24, in_channels=4, out_channels=8, num_layers=2,
                       cross_attention_dim=48, sample_size=8, patch_size=2, caption_channels=64)
    hip = PixArtTransformer2DModelHIP(cfg, device=DEV).init_synthetic(4)
    recipe = PixArtRecipe(hip, pad_to=64, device=DEV)
    g = torch.Generator().manual_seed(3)
    latents = (torch.randn(3, cfg.in_channels, 8, 12, generator=g) * 0.5).to(BF)
    embs = [torch.randn(L, cfg.caption_channels, generator=g).to(BF) for L in (5, 64, 17)]

    def seeded(fn):
        torch.manual_seed(11)
        torch.cuda.manual_seed(11)
        out = fn()
        torch.cuda.synchronize()
        return out.detach().clone(), hip.flat_grad.clone()

    def autograd_path(gen=None):
        loss = recipe.optimize(latents, embs, gen)
        loss.backward()
        return loss
    la, ga = seeded(autograd_path)
    for rep in range(3):                                            # the third call replays the recorded plans
        r0 = getattr(hip, "plan_replays", 0)
        ld, gd = seeded(lambda: recipe.optimize_device(latents, embs, None))
        assert ld.dtype == BF and torch.equal(la, ld) and torch.equal(ga, gd), rep
    assert hip.plan_replays - r0 == 2
    lc, gc = seeded(lambda: autograd_path(torch.Generator().manual_seed(7)))
    ld, gd = seeded(lambda: recipe.optimize_device(latents, embs, torch.Generator().manual_seed(7)))
    assert torch.equal(lc, ld) and torch.equal(gc, gd) and not torch.equal(ga, gc)
    _, gh = seeded(lambda: recipe.optimize_device(latents, embs, None, gscale=0.5))
    assert rel(gh, 0.5 * ga.float()) <= 8e-3


def test_pixart_optimize_device_replays_plans_under_changing_captions():
    """``PixArtRecipe.optimize_device`` with launch plans on and off, same seeds: six steps alternating between two latent
    buckets with captions whose lengths change every step (one of them empty in two steps, T = 300).  A recorded plan holds
    the device addresses of the staged segments, so the steps after each bucket's first one replay only if those addresses
    stayed put -- and are bit-identical to the unplanned run only if the staged data landed where the plan reads it."""
    from yat_amd.pixart import PixArtConfig, PixArtTransformer2DModelHIP
    from yat_amd.recipe import PixArtRecipe
    cfg = PixArtConfig(num_attention_heads=2, attention_head_dim=24, in_channels=4, out_channels=8, num_layers=2,
                       cross_attention_dim=48, sample_size=8, patch_size=2, caption_channels=64)
    T, shapes = 300, ((8, 8), (4, 16))
    captions = ((40, 300), (7, 129), (0, 65), (300, 1), (64, 0), (200, 13))          # B = 2 caption lengths per step
    runs = []
    for plans in (False, True):
        hip = PixArtTransformer2DModelHIP(cfg, device=DEV).init_synthetic(4)
        hip.use_plans = plans
        recipe = PixArtRecipe(hip, pad_to=T, device=DEV)
        g = torch.Generator().manual_seed(9)
        torch.manual_seed(21)                     # the timestep draws (global CPU stream) and the noise (global device stream)
        torch.cuda.manual_seed(21)
        losses, nplans = [], []
        for step, lens in enumerate(captions):
            h, w = shapes[step % 2]
            latents = (torch.randn(2, cfg.in_channels, h, w, generator=g) * 0.5).to(BF)
            embs = [torch.randn(L, cfg.caption_channels, generator=g).to(BF) for L in lens]
            losses.append(recipe.optimize_device(latents, embs, None))
            nplans.append(len(hip._plans))
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), hip.flat_grad.clone(), getattr(hip, "plan_replays", 0), nplans))
    (l_off, g_off, r_off, n_off), (l_on, g_on, r_on, n_on) = runs
    print(f"[plans] pixart optimize_device: plans after each step {n_on}, {r_on} replays; losses {l_on.tolist()}")
    assert r_off == 0 and n_off[-1] == 0
    assert torch.isfinite(l_on.float()).all() and torch.equal(l_off, l_on) and torch.equal(g_off, g_on)
    assert r_on >= 2 * 4                                   # steps 2..5: forward and backward replayed
    assert n_on[1] > 0 and n_on[1:] == [n_on[1]] * 5       # nothing recorded after each bucket's first step


def test_pixart_validation_sampler_matches_oracle():
    """CFG + DPM-Solver++ (2M) latent sampler -- the middle third of the reference's PixArt-Sigma ``validate()``
    (train_pixart_sigma.py:117-129 over the vendored denoising loop utils/patch_pixart_sigma_pipeline.py:158-208; the scheduler is
    [RECALL]): schedule tables equal to the oracle's, then the HIP model vs the oracle in bf16 and fp32 from the same initial
    latents over 6 steps (first-order start, second-order multistep, first-order final step) on a tiny configuration."""
    from oracle.pixart_ref import DPMSolverPP2MRef, sample_latents_pixart_ref
    from yat_amd.sampler import sample_latents_pixart
    from yat_amd.scheduler import DPMSolverPP2M
    a, b = DPMSolverPP2M(), DPMSolverPP2MRef()
    a.set_timesteps(20)
    b.set_timesteps(20)
    assert torch.equal(a.timesteps, b.timesteps) and torch.equal(a.sigmas, b.sigmas)
    assert int(a.timesteps[0]) == 999 and int(a.timesteps[-1]) == 50 and float(a.sigmas[-1]) == 0.0 and len(a.sigmas) == 21
    ref_bf, ref_32, hip, _, embs, _ = _setup(dict(num_layers=2), 2, 8, 12, [9, 16], seed=3)
    C = embs[0].shape[1]
    T = 16
    enc = torch.zeros(2, T, C, dtype=BF)
    mask = torch.zeros(2, T, dtype=torch.int64)
    for i, e in enumerate(embs):
        enc[i, :e.shape[0]] = e
        mask[i, :e.shape[0]] = 1
    g = torch.Generator().manual_seed(11)
    neg = torch.zeros_like(enc)
    neg[:, :2] = torch.randn(2, 2, C, generator=g).to(BF)
    nmask = torch.zeros_like(mask)
    nmask[:, :2] = 1
    x0 = torch.randn(2, ref_bf.cfg.in_channels, 8, 12, generator=g).to(BF)
    steps = 6
    out = sample_latents_pixart(hip, enc, mask, neg, nmask, 8, 12, num_inference_steps=steps, guidance_scale=5.0, latents=x0)
    o_bf = sample_latents_pixart_ref(ref_bf, x0, enc, mask, neg, nmask, steps, 5.0, BF)
    o_32 = sample_latents_pixart_ref(ref_32, x0, enc, mask, neg, nmask, steps, 5.0, torch.float32)
    e_hip, e_ref = rel(out, o_32), rel(o_bf, o_32)
    print(f"[parity] pixart sampler: hip_vs_fp32={e_hip:.3e} oracle_bf16_vs_fp32={e_ref:.3e} hip_vs_oracle_bf16={rel(out, o_bf):.3e}")
    assert torch.isfinite(out.float()).all() and out.shape == x0.shape
    assert e_hip <= 1.15 * e_ref + 2e-3
