"""Master-weights optimizer mode, the parts that need no GPU: the C entry point's argument checks, ``FlatAdamW``'s state
in both modes on CPU tensors, the refusal of the sharded step, and the ``master_weights`` config key."""
import glob
import json
import os
from types import SimpleNamespace

import pytest
import torch

from yat_amd import lib as ylib
from yat_amd.common.training_parameters_reader import TrainingParameters

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_master_step_bad_arguments_are_rejected_without_a_gpu(built_lib):
    """yat_adamw_master_step validates before any launch, so fake non-null pointers are never dereferenced."""
    lib = ylib.load()
    P, EINVAL = 0x7f0000001000, -1
    good = dict(n=64, param=P, master=P, grad=P, exp_avg=P, exp_avg_sq=P, step=1)

    def call(**kw):
        a = {**good, **kw}
        return lib.yat_adamw_master_step(a["n"], a["param"], a["master"], a["grad"], a["exp_avg"], a["exp_avg_sq"], None, 1e-4,
                                         0.9, 0.999, 1e-8, 0.0, a["step"], 1, None, 0.0, None)

    assert call(n=7) == EINVAL
    assert call(n=0) == EINVAL
    assert call(n=-8) == EINVAL
    assert call(n=(1 << 33) + 4) == EINVAL            # n % 8 is checked on all 64 bits
    assert call(step=0) == EINVAL
    for name in ("param", "master", "grad", "exp_avg", "exp_avg_sq"):
        assert call(**{name: None}) == EINVAL, name


def _stand_in(**extra):
    """The five-tensor, two-bucket flat layout of tests/test_optim_gpu.py::test_nonfinite_gradient_follows_torch, on the CPU."""
    numel = [96 * 40, 40, 3 * 3 * 16, 2000, 8]
    buckets = [[0, 1], [2, 3, 4]]
    up = lambda x, a: -(-x // a) * a
    starts, lows, off = [], [], 0
    for b in buckets:
        off = up(off, 64)
        lows.append(off)
        for t in b:
            starts.append(off)
            off += up(numel[t], 8)
    off = up(off, 64)
    g = torch.Generator().manual_seed(7)
    return SimpleNamespace(flat_param=(torch.randn(off, generator=g) * 0.5).to(BF), flat_grad=torch.zeros(off, dtype=BF),
                           seg_start=torch.tensor(starts + [off], dtype=torch.int64), numel_flat=off,
                           bucket_bounds=list(zip(lows, lows[1:] + [off])), param_events=None,
                           join_pending_update=lambda: None, **extra)


def test_flat_adamw_master_state(monkeypatch):
    from yat_amd.optim import MASTER_GRID_PASS, FlatAdamW
    monkeypatch.delenv("YAT_MASTER_WEIGHTS", raising=False)
    assert MASTER_GRID_PASS == 8192 * 256 * 8
    model = _stand_in()
    n = model.numel_flat
    opt = FlatAdamW(model, lr=1e-5, master_weights=True, use_ema=True)
    assert opt.master_weights is True
    for name in ("master", "exp_avg", "exp_avg_sq", "ema_shadow"):
        t = getattr(opt, name)
        assert t.dtype == torch.float32 and t.shape == (n,), name
    assert torch.equal(opt.master, model.flat_param.float())
    assert torch.equal(opt.ema_shadow, opt.master) and opt.ema_shadow.data_ptr() != opt.master.data_ptr()
    assert not opt.exp_avg.any() and not opt.exp_avg_sq.any()
    assert model.flat_param.dtype == BF                       # the working copy stays what the kernels read
    model.flat_param.mul_(2.0)
    assert not torch.equal(opt.master, model.flat_param.float())
    opt.resync_master()
    assert torch.equal(opt.master, model.flat_param.float())
    assert FlatAdamW(model, lr=1e-5, master_weights=True).ema_shadow is None


@pytest.mark.parametrize("how", ["false", "unset", "env_0", "env_empty"])
def test_flat_adamw_default_state_is_bf16(monkeypatch, how):
    from yat_amd.optim import FlatAdamW
    monkeypatch.delenv("YAT_MASTER_WEIGHTS", raising=False)
    if how.startswith("env"):
        monkeypatch.setenv("YAT_MASTER_WEIGHTS", "0" if how == "env_0" else "")
    model = _stand_in()
    opt = FlatAdamW(model, lr=1e-5, use_ema=True, **(dict(master_weights=False) if how == "false" else {}))
    assert opt.master_weights is False and opt.master is None
    for name in ("exp_avg", "exp_avg_sq", "ema_shadow"):
        assert getattr(opt, name).dtype == BF and getattr(opt, name).shape == (model.numel_flat,), name
    assert torch.equal(opt.ema_shadow, model.flat_param)
    opt.resync_master()                                       # nothing to do, and no error


def test_environment_variable_selects_the_mode_when_the_argument_is_none(monkeypatch):
    from yat_amd.optim import FlatAdamW
    monkeypatch.setenv("YAT_MASTER_WEIGHTS", "1")
    assert FlatAdamW(_stand_in(), lr=1e-5).master_weights is True
    assert FlatAdamW(_stand_in(), lr=1e-5, master_weights=None).master.dtype == torch.float32
    assert FlatAdamW(_stand_in(), lr=1e-5, master_weights=False).master is None       # an explicit argument wins


def test_sharded_step_with_master_weights_is_refused():
    from yat_amd.optim import FlatAdamW
    model = _stand_in(shard=SimpleNamespace(ddp=None, rank=0, world=2))
    opt = FlatAdamW(model, lr=1e-5, master_weights=True, use_ema=True)
    before = (model.flat_param.clone(), opt.master.clone())
    with pytest.raises(NotImplementedError, match="master_weights"):
        opt.step()
    assert opt.step_count == 0 and torch.equal(model.flat_param, before[0]) and torch.equal(opt.master, before[1])


# ------------------------------------------------------------------------------------------------ config key
BASE = "urls:\n  - a.tar\nbatch_size: 2\nlearning_rate: 1e-5\nsteps: 4\nnum_steps_per_validation: 2\nvalidation_prompts:\n  - x\n"


def _read(tmp_path, extra):
    f = tmp_path / "c.yaml"
    f.write_text(BASE + extra)
    return TrainingParameters().read_yaml(str(f))


@pytest.mark.parametrize("text, want", [("true", True), ("1", True), ("yes", True), ("false", False), ("False", False), ("0", False),
                                        ("no", False), ("off", False)])
def test_config_key_is_parsed_like_shard_optimizer(tmp_path, text, want):
    assert _read(tmp_path, f"master_weights: {text}\n").master_weights is want
    assert _read(tmp_path, f"shard_optimizer: {text}\n").shard_optimizer is want


def test_config_without_the_key_is_unchanged(tmp_path):
    p = _read(tmp_path, "")
    assert not hasattr(p, "master_weights")
    with_key = vars(_read(tmp_path, "master_weights: true\n"))
    assert {k: v for k, v in with_key.items() if k != "master_weights"} == vars(p)
    for path in sorted(glob.glob(os.path.join(GOLDEN, "config_*.yaml"))):       # the reference's configs parse as before
        golden = json.load(open(path.replace("config_", "params_").replace(".yaml", ".json")))
        assert "master_weights" not in golden
        assert json.loads(json.dumps(vars(TrainingParameters().read_yaml(path)))) == golden, path


@pytest.mark.parametrize("key, env, want", [(None, None, False), (None, "1", True), (None, "0", False), ("true", None, True),
                                            ("true", "0", True), ("false", "1", False), ("0", "1", False)])
def test_key_wins_over_the_environment_in_make_optimizer(tmp_path, monkeypatch, key, env, want):
    """``Model.make_optimizer`` hands the key to FlatAdamW; YAT_MASTER_WEIGHTS decides only when the key is absent."""
    from yat_amd.common.trainer import Model, optimizer_arithmetic
    monkeypatch.delenv("YAT_MASTER_WEIGHTS", raising=False)
    if env is not None:
        monkeypatch.setenv("YAT_MASTER_WEIGHTS", env)
    params = _read(tmp_path, "" if key is None else f"master_weights: {key}\nuse_ema: true\n")
    opt = Model.make_optimizer(SimpleNamespace(params=params), _stand_in())
    assert opt.master_weights is want and (opt.master is not None) == want
    assert opt.exp_avg.dtype == (torch.float32 if want else BF)
    assert optimizer_arithmetic(opt).startswith("master_weights" if want else "bf16")
