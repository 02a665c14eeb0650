"""The trainer with ``master_weights: true`` end to end on the GPU (tiny SANA configuration, synthetic cached-feature shards;
the helper restates the one of tests/test_trainer_gpu.py): the bf16 flat buffer stays the rounding of the fp32 master through
steps, the EMA swap of a validation + save and the end of the run; at a learning rate of 1e-6 the master weights move where
the all-bf16 step leaves them; checkpoints keep the bf16 diffusers / peft layout and load."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


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


def _trainer(tmp_path, monkeypatch, extra_yaml, steps, cadence):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from train_sana import SanaModel
    from yat_amd.common.training_parameters_reader import TrainingParameters
    cfg = _tiny_cfg()
    tmp_path.mkdir(exist_ok=True)
    paths = _write_shards(tmp_path, cfg)
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", *[f"  - {p}" for p in paths], "num_shards: 2", "dataset_seed: 7",
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
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    return SanaModel(params, config=cfg), cfg, yaml_path


def _is_rounding_of(flat_bf16, master):
    return torch.equal(flat_bf16.view(torch.int16), master.to(BF).view(torch.int16))


def test_full_model_run_with_master_weights(tmp_path, monkeypatch, capsys):
    from safetensors.torch import load_file
    from yat_amd.sana import SanaTransformer2DModelHIP
    # validation + save at global steps 0 and 4 of 6 (the cadence test of common/trainer.py:371 holds at step 0 too)
    trainer, cfg, _ = _trainer(tmp_path / "master", monkeypatch, ["use_ema: true", "master_weights: true"], steps=6, cadence=4)
    before = trainer.model.flat_param.clone()
    saves, inner = [], trainer._validate_and_save

    def checked():
        inner()
        opt = trainer.optimizer
        trainer.model.join_pending_update()
        torch.cuda.synchronize()
        saves.append((trainer.global_step, _is_rounding_of(trainer.model.flat_param, opt.master), opt.ema_shadow.clone()))
    trainer._validate_and_save = checked
    trainer.run()
    trainer.model.join_pending_update()
    torch.cuda.synchronize()
    opt = trainer.optimizer
    assert "optimizer arithmetic: master_weights" in capsys.readouterr().out
    assert opt.master_weights and opt.master.dtype == torch.float32 and opt.ema_shadow.dtype == torch.float32
    assert trainer.ema_model is opt.ema_shadow
    losses = [float(l) for l in trainer.loss_history]
    assert len(losses) == 6 and all(torch.isfinite(torch.tensor(losses))), losses
    assert [s for s, _, _ in saves] == [0, 4]
    assert all(ok for _, ok, _ in saves), "the EMA swap of a validation + save did not put bf16(master) back"
    assert _is_rounding_of(trainer.model.flat_param, opt.master), "flat_param is not bf16(master) after the run"
    assert not torch.equal(opt.ema_shadow, opt.master)

    # at lr 1e-6 the master moves wherever a gradient arrived ...
    touched = opt.exp_avg != 0
    assert touched.any()
    moved_master = (opt.master != before.float())[touched].float().mean().item()
    moved_copy = (trainer.model.flat_param != before)[touched].float().mean().item()

    # ... the checkpoint of step 4 is bf16(EMA shadow at that save) in the diffusers layout, and loads
    step, _, shadow = saves[-1]
    ck = tmp_path / "master" / "models" / str(step)
    assert json.loads((ck / "config.json").read_text())["_class_name"] == "SanaTransformer2DModel"
    sd = load_file(str(ck / "diffusion_pytorch_model.safetensors"))
    assert sd and all(v.dtype == BF for v in sd.values())
    re = SanaTransformer2DModelHIP.from_pretrained(str(ck), device="cuda")
    assert re.flat_param.dtype == BF and _is_rounding_of(re.flat_param, shadow), "the checkpoint is not bf16(ema_shadow)"
    del re

    # ... and the same run without the key leaves most of those bf16 weights where they were
    plain, _, _ = _trainer(tmp_path / "plain", monkeypatch, ["use_ema: true"], steps=6, cadence=4)
    before_plain = plain.model.flat_param.clone()
    assert torch.equal(before_plain, before)
    plain.run()
    plain.model.join_pending_update()
    torch.cuda.synchronize()
    assert "optimizer arithmetic: bf16" in capsys.readouterr().out
    assert not plain.optimizer.master_weights and plain.optimizer.master is None and plain.optimizer.exp_avg.dtype == BF
    moved_plain = (plain.model.flat_param != before_plain)[touched].float().mean().item()
    print(f"[master] 6 steps at lr 1e-6, {int(touched.sum())} of {touched.numel()} elements with a gradient: moved in the fp32 master "
          f"{moved_master:.4f}, in its bf16 working copy {moved_copy:.4f}, in the all-bf16 run {moved_plain:.4f}")
    assert moved_master >= 0.99
    assert (opt.master != before.float())[touched].sum().item() > (plain.model.flat_param != before_plain)[touched].sum().item()


def test_lora_run_with_master_weights(tmp_path, monkeypatch):
    from safetensors.torch import load_file
    from train_sana import SanaModel
    from yat_amd.common.training_parameters_reader import TrainingParameters
    targets = ["conv_inverted", "conv_point", "to_q", "to_k", "to_v", "to_out.0", "linear_1", "linear_2", "proj"]
    extra = ["lora_rank: 8", "lora_alpha: 8", "lora_algo: lora", "lora_target_modules:", *[f"  - {t}" for t in targets],
             "master_weights: true"]
    trainer, cfg, yaml_path = _trainer(tmp_path / "lora", monkeypatch, extra, steps=3, cadence=2)
    base = trainer.model.flat_param.clone()
    trainer.run()
    trainer.adapters.join_pending_update()
    torch.cuda.synchronize()
    opt = trainer.optimizer
    assert trainer.adapters is not None and opt.model is trainer.adapters and opt.master_weights
    assert len(trainer.loss_history) == 3 and all(torch.isfinite(torch.tensor([float(l) for l in trainer.loss_history])))
    assert opt.master.dtype == torch.float32 and opt.master.numel() == trainer.adapters.flat_param.numel()
    assert _is_rounding_of(trainer.adapters.flat_param, opt.master), "the adapter set's flat_param is not bf16(master)"
    assert (opt.exp_avg != 0).any()
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
    # a restarted run re-derives its master from the bf16 adapter it loaded (the load happens before the optimizer is made)
    assert torch.equal(resumed.optimizer.master, resumed.adapters.flat_param.float())
