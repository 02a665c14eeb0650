"""SANA-1.5 (``qk_norm="rms_norm_across_heads"``) end to end on the GPU: the training step against the CPU reference of
tests/sana15_ref.py, launch plans, checkpoint round trip, LoRA, the sampler, and the SANA-1.0 guard.

Step parity is the procedure and the bars of tests/test_sana_gpu.py::test_step_matches_oracle (its docstring derives them), all
relative to the reference's own bf16 error against its fp32 run: loss 1.1 x + 1e-3, prediction and all-parameter gradients
1.1 x + 1e-3, every parameter 2.0 x + 2e-2, clip + AdamW within 1 bf16 ulp on >= 99 % of the elements.  The LoRA case uses the
bars of tests/test_lora_gpu.py (1.15 x + 2e-3 loss and adapter gradients, 1.15 x + 1e-3 prediction).

The SANA-1.0 guard.  With ``qk_norm=None`` this file checks what can be checked inside one tree: no segmented-norm launch, no
q/k buffer in the arena, the parent's launch sequence length.  The comparison against the parent commit itself was run by hand,
once, on an MI355X: the parent tree and this tree, each with its own library, each in a fresh process, ran the same seeded step
of a tiny SANA-1.0 model (3 blocks, block 1 with softmax self-attention, B = 3, 6 x 10 latents, prompts of 7 / 40 / 1 rows,
packed and padded text, eager and replayed from a launch plan); loss, prediction and the flat gradient buffer were bit-identical
in all four runs.
"""
import copy

import pytest
import torch

from tests.sana15_ref import SanaTransformer15Ref, hip_config, init_like_pretrained15

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEV = "cuda"
NORM_KEYS = ("attn1.norm_q.weight", "attn1.norm_k.weight", "attn2.norm_q.weight", "attn2.norm_k.weight")


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def _tiny(**kw):
    from oracle.sana_ref import SanaConfig as RefCfg
    return RefCfg.tiny(**kw)


def _setup(cfg_kw, B, h, w, lens, seed=0):
    from yat_amd.sana import SanaTransformer2DModelHIP
    rcfg = _tiny(**cfg_kw)
    ref = SanaTransformer15Ref(rcfg)
    init_like_pretrained15(ref, seed)
    ref_bf = copy.deepcopy(ref).to(BF)
    ref_32 = copy.deepcopy(ref_bf).float()          # same (bf16-representable) weights, fp32 arithmetic
    hip = SanaTransformer2DModelHIP(hip_config(rcfg), device=DEV)
    hip.load_state_dict(ref_bf.state_dict())
    g = torch.Generator().manual_seed(100 + seed)
    latents = (torch.randn(B, rcfg.in_channels, h, w, generator=g) * 0.5).to(BF)
    embs = [torch.randn(L, rcfg.caption_channels, generator=g).to(BF) for L in lens]
    return ref_bf, ref_32, hip, latents, embs


@pytest.mark.parametrize("B,h,w,lens,pad_to,layers,modified", [
    (2, 4, 4, [5, 16], 16, 2, []),
    (3, 6, 10, [7, 40, 1], 64, 2, []),
    (2, 6, 10, [7, 40], 64, 3, [0, 2]),          # blocks 0 and 2 with softmax self-attention (modified_blocks)
])
def test_step_matches_oracle(B, h, w, lens, pad_to, layers, modified):
    from oracle.recipe_ref import FlowMatchSchedule as RefSched, optimize_ref
    from yat_amd.recipe import SanaRecipe
    from yat_amd.scheduler import FlowMatchSchedule
    from yat_amd.optim import FlatAdamW
    ref_bf, ref_32, hip, latents, embs = _setup(dict(num_layers=layers, modified_blocks=list(modified)), B, h, w, lens)
    sched = RefSched()
    loss_bf, pred_bf, _ = optimize_ref(ref_bf, sched, latents, embs, torch.Generator(), pad_to, BF)
    loss_32, pred_32, _ = optimize_ref(ref_32, sched, latents, embs, torch.Generator(), pad_to, torch.float32)
    loss_bf.backward()
    loss_32.backward()

    recipe = SanaRecipe(hip, FlowMatchSchedule(), pad_to=pad_to, device=DEV)
    loss, pred, _ = recipe.optimize(latents, embs, torch.Generator(), return_pred=True)
    loss.backward()
    torch.cuda.synchronize()

    l_h, l_b, l_t = loss.item(), loss_bf.item(), loss_32.item()
    print(f"[parity] loss hip={l_h:.6f} oracle_bf16={l_b:.6f} oracle_fp32={l_t:.6f}")
    assert abs(l_h - l_t) <= 1.1 * abs(l_b - l_t) + 1e-3 * abs(l_t)
    e_h, e_b, e_hb = rel(pred, pred_32), rel(pred_bf, pred_32), rel(pred, pred_bf)
    print(f"[parity] pred  hip_vs_fp32={e_h:.3e} oracle_bf16_vs_fp32={e_b:.3e} hip_vs_oracle_bf16={e_hb:.3e}")
    assert e_h <= 1.1 * e_b + 1e-3

    # gradients, every parameter tensor -- the four norm weights of every block among them, by name
    p32 = dict(ref_32.named_parameters())
    worst = []
    num_h = num_b = den = 0.0
    for name, pb in ref_bf.named_parameters():
        gh, gb, gt = hip.G[name].float().cpu(), pb.grad.float(), p32[name].grad.float()
        assert torch.isfinite(gh).all(), name
        num_h += (gh - gt).pow(2).sum().item()
        num_b += (gb - gt).pow(2).sum().item()
        den += gt.pow(2).sum().item()
        worst.append((rel(gh, gt), rel(gb, gt), name))
    tot_h, tot_b = (num_h / den) ** 0.5, (num_b / den) ** 0.5
    print(f"[parity] grads (all params) hip_vs_fp32={tot_h:.3e} oracle_bf16_vs_fp32={tot_b:.3e}")
    for eh, eb, name in sorted(worst, reverse=True)[:8]:
        print(f"[parity]   {name}: hip={eh:.3e} oracle_bf16={eb:.3e}")
    assert tot_h <= 1.1 * tot_b + 1e-3
    for eh, eb, name in worst:
        assert eh <= 2.0 * eb + 2e-2, (name, eh, eb)
    checked = {name for _, _, name in worst}
    for i in range(layers):
        for k in NORM_KEYS:
            name = f"transformer_blocks.{i}.{k}"
            assert name in checked and p32[name].grad.abs().max() > 0, name
            eh, eb = next((a, b) for a, b, n in worst if n == name)
            print(f"[parity]   {name}: hip={eh:.3e} oracle_bf16={eb:.3e}")

    # one clip + AdamW step against torch's CPU optimizer fed with the ORACLE's bf16 gradients
    opt_ref = torch.optim.AdamW(ref_bf.parameters(), lr=1e-3, weight_decay=0.01)
    total = torch.nn.utils.clip_grad_norm_(ref_bf.parameters(), max_norm=1.0)
    opt_ref.step()
    opt = FlatAdamW(hip, lr=1e-3, weight_decay=0.01)
    opt.step()
    torch.cuda.synchronize()
    gn = opt.grad_norm.item()
    print(f"[parity] grad norm hip={gn:.5f} torch={total.item():.5f}")
    assert abs(gn - total.float().item()) <= 2e-2 * total.float().item()
    n_bad = n_all = 0
    for name, pb in ref_bf.named_parameters():
        a, b = hip.P[name].float().cpu(), pb.data.float()
        ulp = 2.0 ** -7 * b.abs().clamp_min(1e-30)
        n_bad += ((a - b).abs() > ulp).sum().item()
        n_all += b.numel()
    print(f"[parity] AdamW: {n_bad}/{n_all} parameters differ by more than 1 bf16 ulp from torch CPU")
    assert n_bad <= 0.01 * n_all


@pytest.mark.parametrize("pack", ["1", "0"])
def test_launch_plan_replay_is_bit_identical(pack, monkeypatch):
    """tests/test_sana_gpu.py::test_launch_plan_replay_is_bit_identical on a 1.5 model, with packed and with padded text: eight
    optimizer steps alternating between two buckets with text lengths changing every step -- the row count of attn2.norm_k's
    launches is then a dynamic integer of the plan -- give bit-identical losses and parameters with plans on and off."""
    from yat_amd.recipe import SanaRecipe
    from yat_amd.optim import FlatAdamW
    from yat_amd.sana import SanaTransformer2DModelHIP
    monkeypatch.setenv("YAT_TEXT_PACK", pack)
    rcfg = _tiny(num_layers=3, modified_blocks=[1])
    runs = []
    for plans in (True, False):
        hip = SanaTransformer2DModelHIP(hip_config(rcfg), device=DEV).init_synthetic(4)
        hip.use_plans = plans
        opt = FlatAdamW(hip, lr=1e-3, weight_decay=0.01, overlap_update=True)
        recipe = SanaRecipe(hip, pad_to=128, device=DEV)
        g = torch.Generator().manual_seed(9)
        losses = []
        for step in range(8):
            h, w = ((8, 16), (12, 10))[step % 2]
            latents = (torch.randn(4, rcfg.in_channels, h, w, generator=g) * 0.5).to(BF)
            lens = torch.randint(1, 129, (4,), generator=g).tolist()
            embs = [torch.randn(L, rcfg.caption_channels, generator=g).to(BF) for L in lens]
            losses.append(recipe.optimize_device(latents, embs, torch.Generator().manual_seed(100 + step)))
            assert (hip._saved.kv_off is not None) == (pack == "1")
            opt.step()
        hip.join_pending_update()
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), hip.flat_param.clone(), getattr(hip, "plan_replays", 0), len(hip._plans)))
    (l_a, p_a, replays, nplans), (l_b, p_b, r_b, n_b) = runs
    print(f"[plans] pack={pack}: {nplans} plans recorded, {replays} replays; losses {l_a.tolist()}")
    assert r_b == 0 and n_b == 0
    assert replays >= 2 * 4 and nplans <= 8
    assert torch.isfinite(l_a).all() and torch.equal(l_a, l_b) and torch.equal(p_a, p_b)


def test_state_dict_roundtrip_on_the_device(tmp_path):
    from yat_amd.sana import SanaTransformer2DModelHIP
    ref_bf, _, hip, latents, _ = _setup(dict(num_layers=1), 1, 4, 4, [3])
    sd = hip.state_dict()
    assert set(sd) == set(ref_bf.state_dict())
    for k, v in ref_bf.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k
    hip.save_pretrained(str(tmp_path / "m"))
    again = SanaTransformer2DModelHIP.from_pretrained(str(tmp_path / "m"), device=DEV)
    assert again.cfg == hip.cfg and again.cfg.qk_norm == "rms_norm_across_heads"
    assert torch.equal(again.flat_param, hip.flat_param)
    with torch.no_grad():
        enc = torch.zeros(1, 8, ref_bf.cfg.caption_channels, dtype=BF, device=DEV)
        out = again(latents.to(DEV), encoder_hidden_states=enc, timestep=torch.tensor([500.0]),
                    encoder_attention_mask=torch.ones(1, 8, dtype=torch.long)).sample
    assert out.shape == latents.shape and torch.isfinite(out.float()).all()


def test_without_qk_norm_no_norm_is_launched(monkeypatch):
    """The SANA-1.0 guard inside one tree (the comparison against the parent commit: module docstring).  A model without the
    setting never reaches the segmented norm and keeps no q/k buffer; one with it launches, per block, attn1's q|k norm and
    attn2's q norm once per forward chain, attn2's k norm once on the text rows, and the three backward norms once each (the
    backward runs on the whole batch); nothing else differs in the launch sequence."""
    from yat_amd import ops
    from yat_amd.recipe import SanaRecipe
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    rcfg = _tiny(num_layers=2)
    g = torch.Generator().manual_seed(5)
    latents = (torch.randn(2, rcfg.in_channels, 6, 10, generator=g) * 0.5).to(BF)
    embs = [torch.randn(L, rcfg.caption_channels, generator=g).to(BF) for L in (7, 40)]
    calls = []
    real = ops._l.load()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if "_workspace_bytes" in name:
                return fn

            def call(*a):
                calls.append(name)
                return fn(*a)
            return call
    counts = {}
    for tag, cfg in (("1.0", SanaConfig(**{k: getattr(rcfg, k) for k in SanaConfig.__dataclass_fields__})),
                     ("1.5", hip_config(rcfg))):
        hip = SanaTransformer2DModelHIP(cfg, device=DEV).init_synthetic(4)
        hip.use_plans = False
        recipe = SanaRecipe(hip, pad_to=64, device=DEV)
        calls.clear()
        monkeypatch.setattr(ops, "_lib", lambda: Spy())
        loss, _, _ = recipe.optimize(latents, embs, torch.Generator().manual_seed(7), return_pred=True)
        loss.backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert torch.isfinite(loss) and torch.isfinite(hip.flat_grad.float()).all()
        counts[tag] = (calls.count("yat_rmsnorm_seg_fwd"), calls.count("yat_rmsnorm_seg_bwd"),
                       [c for c in calls if "rmsnorm_seg" not in c], sorted(k for k in hip._arena if "raw" in k or "qkn" in k))
    f0, b0, rest0, arena0 = counts["1.0"]
    f1, b1, rest1, arena1 = counts["1.5"]
    assert (f0, b0) == (0, 0) and arena0 == []
    chains = min(hip.fwd_chains, latents.shape[0])
    assert chains == 2                            # (the default schedule: two image-range chains)
    assert (f1, b1) == ((2 * chains + 1) * rcfg.num_layers, 3 * rcfg.num_layers) and len(arena1) == 3 * rcfg.num_layers + 2
    assert rest0 == rest1                         # every other launch, in order, is the 1.0 step's


def test_lora_step_matches_oracle():
    """Rank-8 LoRA on to_q / to_k / to_v of a one-block 1.5 model against oracle/lora_ref.py wrapped around the 1.5 reference
    (bars of tests/test_lora_gpu.py); the frozen base's norm weights receive no gradient and do not move."""
    from oracle.recipe_ref import FlowMatchSchedule as RefSched, optimize_ref
    from oracle.lora_ref import apply_lora, LoRAWrapped
    from yat_amd.recipe import SanaRecipe
    from yat_amd.lora import LoRAAdapters
    from yat_amd.optim import FlatAdamW
    targets, r, alpha = ["to_q", "to_k", "to_v"], 8, 16.0
    ref_bf, _, hip, _, _ = _setup(dict(num_layers=1), 2, 6, 10, [9, 30])
    rcfg = ref_bf.cfg
    ad = LoRAAdapters(hip, targets, r=r, alpha=alpha)
    g = torch.Generator().manual_seed(11)
    for e in ad.entries:                                    # meaningful adapters: lora_B away from its zero init
        _, bt = ad._views(e, ad.flat_param)
        bt[:r].copy_((torch.randn(r, e["out"], generator=g) * 0.05).to(BF))
    wrapped = apply_lora(ref_bf, targets, r=r, alpha=alpha)
    assert sorted(wrapped) == sorted(e["module"] for e in ad.entries) and len(wrapped) == 6
    sd = ad.state_dict()
    for name, w in wrapped.items():
        pre = f"base_model.model.{name}."
        with torch.no_grad():
            w.lora_A.copy_(sd[pre + "lora_A.weight"].cpu())
            w.lora_B.copy_(sd[pre + "lora_B.weight"].cpu())
    ref_32 = copy.deepcopy(ref_bf).float()
    latents = (torch.randn(2, rcfg.in_channels, 6, 10, generator=g) * 0.5).to(BF)
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
    print(f"[parity] 1.5 lora loss hip={lh:.6f} oracle_bf16={lbf:.6f} fp32={l32:.6f}")
    assert abs(lh - l32) <= 1.15 * abs(lbf - l32) + 2e-3 * abs(l32)
    e_h, e_r = rel(pred, outs["fp32"][1]), rel(outs["bf16"][1], outs["fp32"][1])
    print(f"[parity] 1.5 lora pred hip_vs_fp32={e_h:.3e} oracle_bf16_vs_fp32={e_r:.3e}")
    assert e_h <= 1.15 * e_r + 1e-3
    hip_g, bf_g, f_g = [], [], []
    for e in ad.entries:
        ga, gbt = ad._views(e, ad.flat_grad)
        hip_g += [ga[:r].float().flatten().cpu(), gbt[:r].t().float().flatten().cpu()]
        bf_g += [t.float().flatten() for t in outs["bf16"][2][e["module"]]]
        f_g += [t.float().flatten() for t in outs["fp32"][2][e["module"]]]
    hg, bg, fg = torch.cat(hip_g), torch.cat(bf_g), torch.cat(f_g)
    e_h, e_r = rel(hg, fg), rel(bg, fg)
    print(f"[parity] 1.5 lora adapter grads hip_vs_fp32={e_h:.3e} oracle_bf16_vs_fp32={e_r:.3e} (n={hg.numel()})")
    assert torch.isfinite(hg).all() and fg.abs().max() > 0
    assert e_h <= 1.15 * e_r + 2e-3
    for k in NORM_KEYS:                                      # frozen base: dx only through the norms
        assert not hip.G["transformer_blocks.0." + k].any(), k
    before = hip.flat_param.clone()
    p0 = ad.flat_param.clone()
    FlatAdamW(ad, lr=1e-3, weight_decay=0.0, max_grad_norm=1.0).step()
    torch.cuda.synchronize()
    assert torch.equal(before, hip.flat_param) and not torch.equal(p0, ad.flat_param)


def test_validation_sampler_runs():
    """validate()'s sampler (CFG + flow-match Euler, yat_amd/sampler.py) on a tiny 1.5 model: finite latents, and not the
    latents the same weights give without the q/k norm."""
    from oracle.recipe_ref import pad_embeddings
    from yat_amd.sampler import sample_latents
    from yat_amd.sana import SanaTransformer2DModelHIP
    ref_bf, _, hip, _, embs = _setup(dict(num_layers=2), 2, 6, 10, [9, 30], seed=3)
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(2, ref_bf.cfg.in_channels, 6, 10, generator=g).to(BF)
    enc, mask = pad_embeddings(embs, 32)
    neg = torch.zeros_like(enc)
    neg[:, :2] = torch.randn(2, 2, enc.shape[-1], generator=g).to(BF)
    nmask = torch.zeros_like(mask)
    nmask[:, :2] = 1
    out = sample_latents(hip, enc, mask, neg, nmask, 6, 10, num_inference_steps=4, guidance_scale=5.0, latents=x0)
    assert out.shape == x0.shape and torch.isfinite(out.float()).all()
    plain = SanaTransformer2DModelHIP(hip_config(ref_bf.cfg, qk_norm=None), device=DEV)
    plain.load_state_dict({k: v for k, v in ref_bf.state_dict().items() if not k.endswith(NORM_KEYS)})
    out0 = sample_latents(plain, enc, mask, neg, nmask, 6, 10, num_inference_steps=4, guidance_scale=5.0, latents=x0)
    assert rel(out, out0) > 1e-2
