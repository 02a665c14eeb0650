"""Stop + resume = the uninterrupted run, on bits (config keys ``save_state`` / ``resume_from``, yat_amd/common/trainer_state.py),
on the tiny SANA trainer (the helper restates the one of tests/test_sr_trainer_gpu.py): 2 layers, batch 4, 2 shards x 16 samples,
lr 1e-3 so that bf16 weights really move, ``warmup_steps: 4``, ``use_ema: true``, ``train_unconditional_prob: 0.5`` with an
``empty_embeds.pt``, validation / save every 2 steps, 6 steps.

Run A is 6 uninterrupted steps.  Run B stops after the save of step 2 (``max_steps=3``) and a NEW trainer object resumes it from
``models/2`` to step 6.  Everything the optimizer holds, the last three losses and the files of ``models/4`` must be equal.
"""
import json
import os
import random
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = ["conv_inverted", "conv_point", "to_q", "to_k", "to_v", "to_out.0", "linear_1", "linear_2", "proj"]
ADAPTER = ["lora_dropout: 0.1", "lora_target_modules:", *[f"  - {t}" for t in TARGETS]]
CASES = {
    "bf16": [],
    "master": ["master_weights: true"],
    "sr": ["stochastic_rounding: true"],
    "accum2": ["gradient_accumulation_steps: 2"],
    "lora": ["lora_algo: lora", "lora_rank: 8", "lora_alpha: 8", *ADAPTER],      # rank-8 LoRA with lora_dropout 0.1
    # LoKr: the same key is its module dropout (rank 2: the rank these targets take -- patch_embed.proj is 8 wide)
    "lokr": ["lora_algo: lokr", "lora_rank: 2", "lora_alpha: 2", *ADAPTER],
}


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


def _tiny_cfg(layers=2):
    from yat_amd.sana import SanaConfig
    return SanaConfig(num_layers=layers, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=2,
                      cross_attention_head_dim=64, cross_attention_dim=128, caption_channels=96, in_channels=8, out_channels=8,
                      sample_size=32)


def _trainer(tmp_path, monkeypatch, extra_yaml, layers=2):
    """A trainer whose working directory is ``tmp_path`` (made and filled on the first call; a later call with other keys is the
    next trainer object of the same run)."""
    sys.path.insert(0, ROOT)
    from train_sana import SanaModel
    from yat_amd.common.training_parameters_reader import TrainingParameters
    cfg = _tiny_cfg(layers)
    if not tmp_path.exists():
        tmp_path.mkdir(parents=True)
        _write_shards(tmp_path, cfg)
        g = torch.Generator().manual_seed(1)
        pe = torch.randn(1, 12, cfg.caption_channels, generator=g).to(BF)
        torch.save([(pe, torch.ones(1, 12, dtype=torch.long), torch.zeros(1, 12, cfg.caption_channels, dtype=BF),
                     torch.cat([torch.ones(1, 1, dtype=torch.long), torch.zeros(1, 11, dtype=torch.long)], 1))],
                   tmp_path / "validation_embeds.pt")
        torch.save([torch.randn(7, cfg.caption_channels, generator=g).to(BF)], tmp_path / "empty_embeds.pt")
    paths = [str(tmp_path / f"shard-{s:06d}.tar") for s in range(2)]
    yaml_path = tmp_path / "config.yaml"
    yaml_path.write_text("\n".join([
        "urls:", "  - unused", "local_shard_paths:", *[f"  - {p}" for p in paths], "num_shards: 2", "dataset_seed: 7",
        "batch_size: 4", "learning_rate: 1e-3", "steps: 6", "num_steps_per_validation: 2", "validation_prompts:", "  - x",
        "bfloat16: true", "aspect_ratio: 1024", "warmup_steps: 4", "use_ema: true", "train_unconditional_prob: 0.5",
        "save_state: true", "save_state_keep: 8", *extra_yaml, ""]))
    monkeypatch.chdir(tmp_path)                       # the trainer writes models/<step>/ relative to the cwd
    monkeypatch.setenv("YAT_TENSORBOARD", "0")
    monkeypatch.delenv("YAT_MASTER_WEIGHTS", raising=False)
    monkeypatch.delenv("YAT_STOCHASTIC_ROUNDING", raising=False)
    params = TrainingParameters()
    params.read_yaml(str(yaml_path))
    return SanaModel(params, config=cfg)


def _seed():
    """The trainer seeds neither of the global generators its step draws from (Python's: CFG dropout; torch's: timesteps, adapter
    init and module dropout), as the reference does not: a run that is to be compared starts from a stated seed."""
    random.seed(1234)
    torch.manual_seed(5678)


def _finish(trainer, max_steps=None, fresh=True):
    """run -> what the comparison looks at: every optimizer tensor (clones) and the logged losses"""
    if fresh:
        _seed()
    trainer.run(max_steps=max_steps)
    opt = trainer.optimizer
    opt.model.join_pending_update()
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in opt._state_tensors().items()}
    out["losses"] = torch.stack([l.float() for l in trainer.loss_history]).cpu()
    assert torch.isfinite(out["losses"]).all()
    trainer.sampler.close()
    return out


def _model_files(directory, tensors_only=False):
    """The files of a models/<step> directory (not its trainer_state): tensors, and the JSON files' text"""
    from safetensors.torch import load_file
    out = {}
    for name in sorted(os.listdir(directory)):
        path = os.path.join(directory, name)
        if name.endswith(".safetensors"):
            out.update({f"{name}:{k}": v for k, v in load_file(path).items()})
        elif name == "validation_latents.pt":
            out.update({f"{name}:{i}": v for i, v in enumerate(torch.load(path))})
        elif name.endswith(".json") and not tensors_only:
            out[name] = open(path).read()
    assert any(":" in k for k in out)
    return out


def _same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            x, y = (x[-3:], y[-3:]) if k == "losses" else (x, y)
            assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
            assert torch.equal(x.contiguous().view(torch.uint8).cpu(), y.contiguous().view(torch.uint8).cpu()), (what, k)     # bits
        else:
            assert x == y, (what, k)


def _differs(a, b, keys=None):
    return any(not torch.equal(a[k][-3:] if k == "losses" else a[k], b[k][-3:] if k == "losses" else b[k])
               for k in (keys or a) if torch.is_tensor(a[k]))


def _interrupted(tmp_path, monkeypatch, extra, spoil=None):
    """Run B: three steps (the save of step 2 is its last act), then a new trainer object from ``resume_from``.  ``spoil(t)``
    runs between the restore and the first continued step."""
    first = _trainer(tmp_path, monkeypatch, extra)
    _seed()
    first.run(max_steps=3)
    first.optimizer.model.join_pending_update()
    torch.cuda.synchronize()
    assert sorted(os.listdir(tmp_path / "models")) == ["0", "2"] and first.global_step == 3
    saved = {k: v.clone() for k, v in first.optimizer._state_tensors().items()}
    first.sampler.close()
    del first
    second = _trainer(tmp_path, monkeypatch, extra + [f"resume_from: {tmp_path / 'models' / '2'}"])
    second.initialize()
    assert second.global_step == 3
    _same(saved, {k: v.clone() for k, v in second.optimizer._state_tensors().items()}, "restored state")
    if spoil is not None:
        spoil(second)
    second.initialize = lambda: None               # (already done: run() goes straight on)
    return _finish(second, fresh=False), second


@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    """Run A of every case, made once and left unchanged: {case: (result, directory)}"""
    cache = {}

    def get(case, monkeypatch):
        if case not in cache:
            d = tmp_path_factory.mktemp(f"a_{case}") / "run"
            cache[case] = (_finish(_trainer(d, monkeypatch, CASES[case])), d)
        return cache[case]
    return get


def test_control_two_uninterrupted_runs_give_equal_bits(tmp_path, monkeypatch, run_a):
    a, _ = run_a("bf16", monkeypatch)
    again = _finish(_trainer(tmp_path / "again", monkeypatch, CASES["bf16"]))
    assert len(a["losses"]) == 6
    _same(a, dict(again, losses=again["losses"]), "two uninterrupted runs")
    assert torch.equal(a["losses"], again["losses"])
    assert (a["exp_avg"] != 0).any() and not torch.equal(a["param"], a["ema_shadow"])


@pytest.mark.parametrize("case", list(CASES))
def test_continuation_equals_the_uninterrupted_run(tmp_path, monkeypatch, run_a, case):
    a, a_dir = run_a(case, monkeypatch)
    if case in ("lora", "lokr"):
        control = _finish(_trainer(tmp_path / "control", monkeypatch, CASES[case]))
        if _differs(a, control):
            # the adapter step itself is not bit-stable from run to run: only "the restored state equals the saved one" can be
            # held (asserted inside _interrupted), and the summary says so
            _interrupted(tmp_path / "b", monkeypatch, CASES[case])
            import warnings
            warnings.warn(f"resume, {case}: two uninterrupted runs differ; only restored == saved is held")
            return
    b, second = _interrupted(tmp_path / "b", monkeypatch, CASES[case])
    assert len(b["losses"]) == 3 and second.global_step == 6
    assert ("master" in a) == (case == "master")
    _same(a, b, f"{case}: run A against stop + resume")
    _same(_model_files(a_dir / "models" / "4"), _model_files(tmp_path / "b" / "models" / "4"), f"{case}: models/4")
    sa = json.load(open(a_dir / "models" / "4" / "trainer_state" / "state.json"))
    sb = json.load(open(tmp_path / "b" / "models" / "4" / "trainer_state" / "state.json"))
    for key in ("global_step", "micro_step", "scheduler_last_epoch", "optimizer", "fingerprints"):
        assert sa[key] == sb[key], (case, key)
    assert sa["ranks"]["0"]["python_random"] == sb["ranks"]["0"]["python_random"]


def test_second_half_through_the_command_line(tmp_path, monkeypatch, run_a):
    """``python train_sana.py --config ...`` in a fresh child process with ``resume_from: latest``"""
    from safetensors.torch import load_file
    a, a_dir = run_a("bf16", monkeypatch)
    d = tmp_path / "b"
    first = _trainer(d, monkeypatch, CASES["bf16"])
    first.model.save_pretrained(str(d / "init"))                # the child builds its transformer from a directory, as users do
    _seed()
    first.run(max_steps=3)
    first.optimizer.model.join_pending_update()
    torch.cuda.synchronize()
    first.sampler.close()
    config = d / "config.yaml"
    config.write_text(config.read_text() + f"pretrained_model_path: {d / 'init'}\nresume_from: latest\n")
    env = dict(os.environ, YAT_TENSORBOARD="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_sana.py"), "--config", str(config)], cwd=str(d), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "trainer state: resumed from" in r.stdout and "continuing at 3" in r.stdout
    assert sorted(os.listdir(d / "models")) == ["0", "2", "4"]
    # (tensors: the child's transformer came from a directory, its config.json may spell the same configuration differently)
    _same(_model_files(a_dir / "models" / "4", True), _model_files(d / "models" / "4", True), "models/4 written by the child")
    ta = load_file(str(a_dir / "models" / "4" / "trainer_state" / "optimizer.safetensors"))
    tb = load_file(str(d / "models" / "4" / "trainer_state" / "optimizer.safetensors"))
    _same(ta, tb, "optimizer state at step 4 written by the child")
    ra = load_file(str(a_dir / "models" / "4" / "trainer_state" / "rng_rank0.safetensors"))
    rb = load_file(str(d / "models" / "4" / "trainer_state" / "rng_rank0.safetensors"))
    assert torch.equal(ra["torch_cpu"], rb["torch_cpu"])


def _other_python_rng(t):
    """A Python RNG state whose next three CFG-dropout decisions differ from the restored state's"""
    def decisions(state):
        r = random.Random()
        r.setstate(state)
        return [r.random() < 0.5 for _ in range(3)]
    want = decisions(random.getstate())
    for seed in range(100):
        if decisions(random.Random(seed).getstate()) != want:
            random.seed(seed)
            return
    raise AssertionError("no seed found")


def _other_torch_rng(t):
    """A state of torch's global CPU generator whose module-dropout draws of the next step (one ``torch.rand(1)`` per adapter
    entry) drop another set of adapters than the restored state's.  (In a SANA run nothing else reads that generator: the
    timesteps and the noise come from the step's own fresh generator.)"""
    n, p = len(t.adapters.entries), t.adapters.module_dropout
    assert p > 0

    def drops(g):
        return [bool(torch.rand(1, generator=g) > p) for _ in range(n)]
    g = torch.Generator()
    g.set_state(torch.get_rng_state())
    want = drops(g)
    for seed in range(100):
        if drops(torch.Generator().manual_seed(seed)) != want:
            torch.manual_seed(seed)
            return
    raise AssertionError("no seed found")


def _spoil_sampler(t):
    assert t.sampler._resume is not None
    t.sampler._resume = dict(t.sampler._resume, consumed=t.sampler._resume["consumed"] + 3)


SPOILS = {
    # name: (case, what is done to the restored trainer, tensors that must differ -- None: any)
    "exp_avg zeroed": ("bf16", lambda t: t.optimizer.exp_avg.zero_(), None),
    "exp_avg_sq zeroed": ("bf16", lambda t: t.optimizer.exp_avg_sq.zero_(), None),
    "step_count - 1": ("bf16", lambda t: setattr(t.optimizer, "step_count", t.optimizer.step_count - 1), None),
    "ema_steps reset": ("bf16", lambda t: setattr(t.optimizer, "ema_steps", 0), ["ema_shadow"]),
    "scheduler epoch": ("bf16", lambda t: setattr(t.lr_scheduler, "last_epoch", t.lr_scheduler.last_epoch - 2), None),
    "torch RNG state": ("lokr", _other_torch_rng, None),
    "python RNG state": ("bf16", _other_python_rng, None),
    "sampler cursor": ("bf16", _spoil_sampler, None),
    "master = float(param)": ("master", lambda t: t.optimizer.master.copy_(t.model.flat_param), ["master"]),
    "stochastic-rounding step": ("sr", lambda t: setattr(t.optimizer, "step_count", t.optimizer.step_count - 1), None),
}


@pytest.mark.parametrize("name", list(SPOILS))
def test_each_saved_field_matters(tmp_path, monkeypatch, run_a, name):
    case, spoil, keys = SPOILS[name]
    a, _ = run_a(case, monkeypatch)
    b, _ = _interrupted(tmp_path / "b", monkeypatch, CASES[case], spoil=spoil)
    assert _differs(a, b, keys), f"{name}: the continuation is still run A"


def test_refusals(tmp_path, monkeypatch):
    d = tmp_path / "b"
    first = _trainer(d, monkeypatch, CASES["bf16"])
    _seed()
    first.run(max_steps=3)
    first.optimizer.model.join_pending_update()
    torch.cuda.synchronize()
    first.sampler.close()
    resume = [f"resume_from: {d / 'models' / '2'}"]
    with pytest.raises(ValueError, match="mode 'bf16'.*'master'"):
        _trainer(d, monkeypatch, ["master_weights: true"] + resume).initialize()
    with pytest.raises(ValueError, match="another layout.*entry"):
        _trainer(d, monkeypatch, resume, layers=3).initialize()
    with pytest.raises(ValueError, match="no complete trainer state"):
        _trainer(d, monkeypatch, [f"resume_from: {d / 'models' / '1'}"]).initialize()
    sdir = d / "models" / "2" / "trainer_state"
    meta = json.loads((sdir / "state.json").read_text())
    (sdir / "state.json").write_text(json.dumps({**meta, "world_size": 2}))
    with pytest.raises(ValueError, match="saved by 2 process"):
        _trainer(d, monkeypatch, resume).initialize()
    (sdir / "state.json").write_text(json.dumps(meta))
    raw = bytearray((sdir / "optimizer.safetensors").read_bytes())
    n = int.from_bytes(raw[:8], "little")
    at = 8 + n + json.loads(raw[8:8 + n])["exp_avg"]["data_offsets"][0] + 6
    raw[at] ^= 0x01
    (sdir / "optimizer.safetensors").write_bytes(bytes(raw))
    with pytest.raises(ValueError, match="'exp_avg'.*fingerprint"):           # one byte of one tensor: the check names it
        _trainer(d, monkeypatch, resume).initialize()
    raw[at] ^= 0x01
    (sdir / "optimizer.safetensors").write_bytes(bytes(raw))
    ok = _trainer(d, monkeypatch, resume)
    ok.initialize()
    assert ok.global_step == 3
    import types
    ok.model.shard = types.SimpleNamespace(rank=0, world=2, ddp=None)          # the sharded optimizer step
    with pytest.raises(NotImplementedError, match="sharded"):
        ok.optimizer.state_dict()
    ok.sampler.close()
