"""The trainer with ``stochastic_rounding: true`` end to end on the GPU (tiny SANA configuration, synthetic cached-feature
shards; the helper restates the one of tests/test_master_trainer_gpu.py): all state stays bf16, the checkpoint is the bf16 shadow
and loads, and at a learning rate of 1e-6 -- where the all-bf16 step leaves the weights where they are -- the stochastic
rounding moves them along the direction the fp32 master weights take.

Direction: with d_x = p_x - p0 over the elements that saw a gradient (p_master the fp32 master copy) and
c_x = <d_x, d_master> / <d_master, d_master>, c_sr must be nearer to 1 than to c_plain, and |c_sr - 1| under SR_BAR.
"""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# three times the largest |c_sr - 1| measured over dataset seeds 0, 1, 2 on one MI355X (0.0225, 0.0086, 0.0197:
# profiles/sr_adamw_a_trainer.txt), rounded up to one digit; the cap of 0.5 is not reached
SR_BAR = 0.07


def _write_shards(tmp, cfg, n_shards=2, per=16):
    from yat_amd.common.shards import write_shard
    from yat_amd.common.aspect_ratios import ASPECT_RATIO_1024_BIN
    g = torch.Generator().manual_seed(0)
    paths = []
    for s in range(n_shards):
        samples = []
        for i in range(per):
            r = ["1.0", "0.5", "2.0"][(i + s) % 3]
            H, W = ASPECT_RATIO_1024_BIN[r]
            L = int(torch.randint(3, 40, (1,), generator=g))
            samples.append(dict(__key__=f"{s:03d}{i:05d}", ratio=r,
                                latent=(torch.randn(cfg.in_channels, int(H) // 128, int(W) // 128, generator=g) * 0.5).to(BF),
                                emb=torch.randn(L, cfg.caption_channels, generator=g).to(BF)))
        p = str(tmp / f"shard-{s:06d}.tar")
        write_shard(p, samples)
        paths.append(p)
    return paths


def _tiny_cfg():
    from yat_amd.sana import SanaConfig
    return SanaConfig(num_layers=2, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=2,
                      cross_attention_head_dim=64, cross_attention_dim=128, caption_channels=96, in_channels=8, out_channels=8,
                      sample_size=32)


def _trainer(tmp_path, monkeypatch, extra_yaml, steps, cadence, dataset_seed=7):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from train_sana import SanaModel
    from yat_amd.common.training_parameters_reader import TrainingParameters
    cfg = _tiny_cfg()
    tmp_path.mkdir(exist_ok=True)
    paths = _write_shards(tmp_path, cfg)
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", *[f"  - {p}" for p in paths], "num_shards: 2", f"dataset_seed: {dataset_seed}",
        "batch_size: 4", "learning_rate: 1e-6", f"steps: {steps}", f"num_steps_per_validation: {cadence}", "validation_prompts:",
        "  - x", "bfloat16: true", "aspect_ratio: 1024", "train_unconditional_prob: 0.0", *extra_yaml, ""]))
    g = torch.Generator().manual_seed(1)
    pe = torch.randn(1, 12, cfg.caption_channels, generator=g).to(BF)
    torch.save([(pe, torch.ones(1, 12, dtype=torch.long), torch.zeros(1, 12, cfg.caption_channels, dtype=BF),
                 torch.cat([torch.ones(1, 1, dtype=torch.long), torch.zeros(1, 11, dtype=torch.long)], 1))],
               tmp_path / "validation_embeds.pt")
    monkeypatch.chdir(tmp_path)                       # the trainer writes models/<step>/ relative to the cwd
    monkeypatch.setenv("YAT_TENSORBOARD", "0")
    monkeypatch.delenv("YAT_MASTER_WEIGHTS", raising=False)
    monkeypatch.delenv("YAT_STOCHASTIC_ROUNDING", raising=False)
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    return SanaModel(params, config=cfg), cfg, yaml_path


def _run(trainer):
    trainer.run()
    trainer.model.join_pending_update()
    torch.cuda.synchronize()
    losses = [float(l) for l in trainer.loss_history]
    assert len(losses) == 6 and all(torch.isfinite(torch.tensor(losses))), losses
    return losses


def three_runs(tmp_path, monkeypatch, capsys, dataset_seed):
    """6 steps at lr 1e-6 with the EMA shadow, three times from equal weights: stochastic rounding, master weights, neither.
    -> dict of what the test asserts on (also what the profile record of the three seeds was made from)."""
    from safetensors.torch import load_file
    from yat_amd.sana import SanaTransformer2DModelHIP
    out = {}
    sr, cfg, _ = _trainer(tmp_path / "sr", monkeypatch, ["use_ema: true", "stochastic_rounding: true"], 6, 4, dataset_seed)
    p0 = sr.model.flat_param.clone()
    saves, inner = [], sr._validate_and_save

    def checked():
        inner()
        sr.model.join_pending_update()
        torch.cuda.synchronize()
        saves.append((sr.global_step, sr.optimizer.ema_shadow.clone()))
    sr._validate_and_save = checked
    out["loss_sr"] = _run(sr)
    opt = sr.optimizer
    assert "optimizer arithmetic: stochastic_rounding (" in capsys.readouterr().out
    assert opt.stochastic_rounding and not opt.master_weights and opt.master is None and opt.sr_seed == dataset_seed
    for name in ("exp_avg", "exp_avg_sq", "ema_shadow"):
        assert getattr(opt, name).dtype == BF, name
    assert sr.model.flat_param.dtype == BF and sr.ema_model is opt.ema_shadow
    assert [s for s, _ in saves] == [0, 4]
    assert not torch.equal(opt.ema_shadow, sr.model.flat_param)

    # the checkpoint of step 4 is the bf16 shadow at that save in the diffusers layout, and loads
    step, shadow = saves[-1]
    ck = tmp_path / "sr" / "models" / str(step)
    assert json.loads((ck / "config.json").read_text())["_class_name"] == "SanaTransformer2DModel"
    sd = load_file(str(ck / "diffusion_pytorch_model.safetensors"))
    assert sd and all(v.dtype == BF for v in sd.values())
    re = SanaTransformer2DModelHIP.from_pretrained(str(ck), device="cuda")
    assert re.flat_param.dtype == BF and torch.equal(re.flat_param.view(torch.int16), shadow.view(torch.int16)), \
        "the checkpoint is not the bf16 EMA shadow"
    del re

    master, _, _ = _trainer(tmp_path / "master", monkeypatch, ["use_ema: true", "master_weights: true"], 6, 4, dataset_seed)
    assert torch.equal(master.model.flat_param, p0)
    out["loss_master"] = _run(master)
    assert "optimizer arithmetic: master_weights" in capsys.readouterr().out
    plain, _, _ = _trainer(tmp_path / "plain", monkeypatch, ["use_ema: true"], 6, 4, dataset_seed)
    assert torch.equal(plain.model.flat_param, p0)
    out["loss_plain"] = _run(plain)
    assert "optimizer arithmetic: bf16" in capsys.readouterr().out
    assert not plain.optimizer.stochastic_rounding and not plain.optimizer.master_weights

    touched = master.optimizer.exp_avg != 0
    assert touched.any()
    base = p0.double()[touched]
    d_master = master.optimizer.master.double()[touched] - base
    d_sr = sr.model.flat_param.double()[touched] - base
    d_plain = plain.model.flat_param.double()[touched] - base
    mm = (d_master * d_master).sum()
    out["c_sr"], out["c_plain"] = ((d_sr * d_master).sum() / mm).item(), ((d_plain * d_master).sum() / mm).item()
    out["moved_sr"] = (d_sr != 0).float().mean().item()
    out["moved_plain"] = (d_plain != 0).float().mean().item()
    out["moved_master"] = (d_master != 0).float().mean().item()
    out["touched"] = int(touched.sum())
    print(f"[sr] dataset_seed {dataset_seed}: c_sr {out['c_sr']:.4f} (|c_sr - 1| {abs(out['c_sr'] - 1):.4f}), c_plain {out['c_plain']:.4f}; "
          f"moved of {out['touched']} elements with a gradient: sr {out['moved_sr']:.4f}, plain {out['moved_plain']:.4f}, fp32 master "
          f"{out['moved_master']:.4f}; last loss sr {out['loss_sr'][-1]:.5f} master {out['loss_master'][-1]:.5f} plain {out['loss_plain'][-1]:.5f}")
    return out


@pytest.mark.parametrize("dataset_seed", [0, 1, 2])
def test_full_model_run_with_stochastic_rounding(tmp_path, monkeypatch, capsys, dataset_seed):
    r = three_runs(tmp_path, monkeypatch, capsys, dataset_seed)
    assert abs(r["c_sr"] - 1.0) < abs(r["c_sr"] - r["c_plain"]), "the rounded run is nearer to the all-bf16 run than to the master weights"
    assert abs(r["c_sr"] - 1.0) < SR_BAR


def test_lora_run_with_stochastic_rounding(tmp_path, monkeypatch):
    from safetensors.torch import load_file
    from train_sana import SanaModel
    from yat_amd.common.training_parameters_reader import TrainingParameters
    targets = ["conv_inverted", "conv_point", "to_q", "to_k", "to_v", "to_out.0", "linear_1", "linear_2", "proj"]
    extra = ["lora_rank: 8", "lora_alpha: 8", "lora_algo: lora", "lora_target_modules:", *[f"  - {t}" for t in targets],
             "stochastic_rounding: true"]
    trainer, cfg, yaml_path = _trainer(tmp_path / "lora", monkeypatch, extra, steps=3, cadence=2)
    base = trainer.model.flat_param.clone()
    trainer.run()
    trainer.adapters.join_pending_update()
    torch.cuda.synchronize()
    opt = trainer.optimizer
    assert trainer.adapters is not None and opt.model is trainer.adapters and opt.stochastic_rounding and opt.master is None
    assert len(trainer.loss_history) == 3 and all(torch.isfinite(torch.tensor([float(l) for l in trainer.loss_history])))
    assert opt.exp_avg.dtype == BF and opt.exp_avg.numel() == trainer.adapters.flat_param.numel() and (opt.exp_avg != 0).any()
    assert torch.equal(base.view(torch.int16), trainer.model.flat_param.view(torch.int16)), "the frozen base moved"
    ck = tmp_path / "lora" / "models" / "2"
    sd = load_file(str(ck / "adapter_model.safetensors"))
    conf = json.loads((ck / "adapter_config.json").read_text())
    assert conf["peft_type"] == "LORA" and conf["r"] == 8 and all(v.dtype == BF for v in sd.values())
    yaml_path.write_text(yaml_path.read_text() + f"lora_pretrained: {ck}\n")
    params2 = TrainingParameters()
    params2.read_yaml(str(yaml_path))
    resumed = SanaModel(params2, config=cfg)
    resumed.initialize()
    for k, v in resumed.adapters.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    assert resumed.optimizer.stochastic_rounding and resumed.optimizer.sr_seed == 7
