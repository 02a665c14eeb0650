"""The resumable trainer state (yat_amd/common/trainer_state.py) without a GPU: the three config keys, the state directory's
write order, ``latest``, pruning, the refusal of pickles and of a damaged tensor file, and a save -> load round trip of a
host-side optimizer (the host restatement of the fingerprint stands in for the HIP kernel on host tensors)."""
import json
import os
import pickle
import random
import types

import pytest
import torch

from yat_amd.common import trainer_state as ts
from yat_amd.common.trainer import HipAccelerator, WarmupLR
from yat_amd.common.training_parameters_reader import TrainingParameters
from yat_amd.optim import FlatAdamW

BASE_YAML = ["urls:", "  - unused", "batch_size: 4", "learning_rate: 1e-4", "steps: 10", "num_steps_per_validation: 5",
             "validation_prompts:", "  - x"]


def _params(tmp_path, extra):
    p = tmp_path / "config.yaml"
    p.write_text("\n".join(BASE_YAML + extra + [""]))
    return TrainingParameters().read_yaml(str(p))


def test_the_reader_sets_the_keys_only_when_present(tmp_path):
    plain = _params(tmp_path, [])
    for name in ("save_state", "save_state_keep", "resume_from"):
        assert not hasattr(plain, name), name
    on = _params(tmp_path, ["save_state: true", "save_state_keep: 3", "resume_from: latest"])
    assert on.save_state is True and on.save_state_keep == 3 and on.resume_from == "latest"
    assert set(vars(on)) - set(vars(plain)) == {"save_state", "save_state_keep", "resume_from"}
    assert _params(tmp_path, ["save_state: false"]).save_state is False
    assert _params(tmp_path, ["resume_from: models/40"]).resume_from == "models/40"


class _Sampler:
    def __init__(self):
        self.state = {"cursor": 0}

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, s):
        self.state = dict(s)


def _tiny_model(layers=2):
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    m = SanaTransformer2DModelHIP(SanaConfig(num_layers=layers, num_attention_heads=2, num_cross_attention_heads=2,
                                             cross_attention_head_dim=32, cross_attention_dim=64, caption_channels=96,
                                             in_channels=8, out_channels=8, sample_size=4), device="cpu")
    m.flat_param.copy_(torch.randn(m.numel_flat, generator=torch.Generator().manual_seed(1)) * 0.1)
    return m


def _trainer(keep=1, layers=2, **opt_kw):
    t = types.SimpleNamespace()
    t.accelerator = HipAccelerator(2, device="cpu")
    t.model = _tiny_model(layers)
    t.optimizer = FlatAdamW(t.model, lr=1e-3, use_ema=True, **opt_kw)
    t.lr_scheduler = WarmupLR(t.optimizer, 4)
    t.sampler = _Sampler()
    t.params = types.SimpleNamespace(save_state_keep=keep)
    t.logger, t.global_step = None, 0
    return t


def _advance(t, step):
    """stand-in for training up to ``step``: every saved field gets a value of its own"""
    g = torch.Generator().manual_seed(step)
    opt = t.optimizer
    for buf in (t.model.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.ema_shadow):
        buf.copy_(torch.randn(buf.numel(), generator=g))
    if opt.master is not None:
        opt.master.copy_(torch.randn(opt.master.numel(), generator=g))
        t.model.flat_param.copy_(opt.master)                       # bf16(master)
    opt.step_count, opt.ema_steps = step + 1, step + 1
    for _ in range(step + 1 - t.lr_scheduler.last_epoch):
        t.lr_scheduler.step()
    t.accelerator._micro = 2 * (step + 1) + 1
    t.sampler.state = {"cursor": 4 * step}
    t.global_step = step
    random.seed(100 + step)
    torch.manual_seed(200 + step)
    os.makedirs(f"models/{step}", exist_ok=True)
    with open(f"models/{step}/diffusion_pytorch_model.safetensors", "wb") as f:
        f.write(b"model file of step %d" % step)


def test_round_trip_write_order_latest_and_pruning(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    order, real_replace = [], os.replace
    monkeypatch.setattr(ts.os, "replace", lambda a, b: (order.append(os.path.basename(b)), real_replace(a, b))[1])
    a = _trainer(keep=2, master_weights=True)
    assert ts.resolve("latest") is None                                # nothing yet: a fresh start
    for step in (0, 2, 4):
        _advance(a, step)
        order.clear()
        ts.save(a)
        assert order[-1] == "state.json" and set(order[:-1]) == {"rng_rank0.safetensors", "rank0.json", "optimizer.safetensors"}
    # save_state_keep: 2 -- the oldest state is gone, every model file stays
    assert not os.path.exists("models/0/trainer_state") and ts.is_complete("models/2") and ts.is_complete("models/4")
    for step in (0, 2, 4):
        assert open(f"models/{step}/diffusion_pytorch_model.safetensors", "rb").read() == b"model file of step %d" % step
    assert ts.find_latest() == os.path.join("models", "4") and ts.resolve("latest") == os.path.join("models", "4")
    want_py, want_torch = random.getstate(), torch.get_rng_state()
    meta = json.load(open("models/4/trainer_state/state.json"))
    assert meta["format_version"] == 1 and meta["global_step"] == 4 and meta["world_size"] == 1 and meta["micro_step"] == 11
    assert meta["scheduler_last_epoch"] == 5 and meta["optimizer"]["mode"] == "master" and meta["optimizer"]["step_count"] == 5
    assert set(meta["fingerprints"]) == {"param", "exp_avg", "exp_avg_sq", "ema_shadow", "master"}
    assert meta["fingerprints"]["master"] == f"{ts.fingerprint_host(a.optimizer.master):016x}"
    assert len(meta["optimizer"]["layout_sha256"]) == 64 and meta["ranks"]["0"]["sampler"] == {"cursor": 16}

    b = _trainer(master_weights=True)
    random.seed(1), torch.manual_seed(1)
    times = ts.load(b, "models/4")
    assert set(times) >= {"h2d_s", "fingerprint_s", "total_s"}
    assert b.global_step == 5 and b.accelerator._micro == 11 and b.lr_scheduler.last_epoch == 5 and b.sampler.state == {"cursor": 16}
    for name, t in a.optimizer._state_tensors().items():
        got = b.optimizer._state_tensors()[name]
        assert got.dtype == t.dtype and torch.equal(got.view(torch.uint8), t.view(torch.uint8)), name
    assert b.optimizer.step_count == 5 and b.optimizer.ema_steps == 5 and b.optimizer.param_groups[0]["lr"] == 1e-3
    assert random.getstate() == want_py and torch.equal(torch.get_rng_state(), want_torch)


def test_a_directory_without_state_json_is_no_state(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a = _trainer(keep=5)
    _advance(a, 2)
    ts.save(a)
    _advance(a, 4)
    real = ts._write_json

    def killed(path, obj):
        if os.path.basename(path) == "state.json":
            raise KeyboardInterrupt("killed before the state was whole")
        real(path, obj)
    monkeypatch.setattr(ts, "_write_json", killed)
    with pytest.raises(KeyboardInterrupt):
        ts.save(a)
    left = set(os.listdir("models/4/trainer_state"))
    assert "optimizer.safetensors" in left and "state.json" not in left
    assert not ts.is_complete("models/4")
    assert ts.find_latest() == os.path.join("models", "2")              # `latest` skips the unfinished one
    with pytest.raises(ValueError, match="no complete trainer state"):
        ts.resolve("models/4")                                          # ... and naming it is an error
    with pytest.raises(ValueError, match="no complete trainer state"):
        ts.load(_trainer(), "models/4")
    with pytest.raises(ValueError, match="no complete trainer state"):
        ts.resolve("models/7")
    # a state that is being rewritten stops being one first
    monkeypatch.setattr(ts, "_write_json", killed)
    _advance(a, 2)
    with pytest.raises(KeyboardInterrupt):
        ts.save(a)
    assert ts.find_latest() is None


def test_no_state_file_is_a_pickle_and_the_loader_rejects_one(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a = _trainer()
    _advance(a, 2)
    ts.save(a)
    sdir = "models/2/trainer_state"
    names = sorted(os.listdir(sdir))
    assert names == ["optimizer.safetensors", "rank0.json", "rng_rank0.safetensors", "state.json"]
    for n in names:
        raw = open(os.path.join(sdir, n), "rb").read()
        assert raw[:2] != b"PK" and raw[:2] != b"\x1f\x8b", n           # not torch.save's zip, not gzip
        if n.endswith(".json"):
            assert raw[:1] == b"{"                                      # (a pickle starts with 0x80)
            json.loads(raw)
        else:
            size = int.from_bytes(raw[:8], "little")                    # safetensors: the header's length, a JSON object, then
            header = json.loads(raw[8:8 + size])                        # exactly the bytes the header describes: no pickle fits
            assert raw[8:9] == b"{" and max(v["data_offsets"][1] for k, v in header.items() if k != "__metadata__") == len(raw) - 8 - size
    good = open(os.path.join(sdir, "optimizer.safetensors"), "rb").read()
    for name, payload in (("optimizer.safetensors", None), ("rng_rank0.safetensors", None), ("state.json", pickle.dumps({"a": 1}))):
        path = os.path.join(sdir, name)
        keep = open(path, "rb").read()
        if payload is None:
            torch.save({"param": torch.zeros(4)}, path)                  # a zip holding a pickle
        else:
            open(path, "wb").write(payload)
        with pytest.raises(ValueError, match="zip / pickle"):
            ts.load(_trainer(), "models/2")
        open(path, "wb").write(keep)
    assert open(os.path.join(sdir, "optimizer.safetensors"), "rb").read() == good
    ts.load(_trainer(), "models/2")                                      # restored: loads again
    assert "torch.load" not in open(ts.__file__).read() and "import pickle" not in open(ts.__file__).read()


def test_refusals(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a = _trainer()
    _advance(a, 2)
    ts.save(a)
    sdir = "models/2/trainer_state"
    # one byte of a tensor changed: the fingerprint check names the tensor
    path = os.path.join(sdir, "optimizer.safetensors")
    raw = bytearray(open(path, "rb").read())
    header = json.loads(raw[8:8 + int.from_bytes(raw[:8], "little")])
    lo = 8 + int.from_bytes(raw[:8], "little") + header["exp_avg_sq"]["data_offsets"][0]
    raw[lo + 5] ^= 0x10
    open(path, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="'exp_avg_sq'.*fingerprint"):
        ts.load(_trainer(), "models/2")
    raw[lo + 5] ^= 0x10
    open(path, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="mode 'bf16'.*'master'"):
        ts.load(_trainer(master_weights=True), "models/2")
    with pytest.raises(ValueError, match="mode 'bf16'.*'sr'"):
        ts.load(_trainer(stochastic_rounding=True), "models/2")
    with pytest.raises(ValueError, match="another layout.*entry"):
        ts.load(_trainer(layers=3), "models/2")
    other = _trainer()
    other.accelerator.num_processes = 2
    with pytest.raises(ValueError, match="saved by 1 process"):
        ts.load(other, "models/2")
    meta_path = os.path.join(sdir, "state.json")
    meta = json.load(open(meta_path))
    open(meta_path, "w").write(json.dumps({**meta, "format_version": 99}))
    with pytest.raises(ValueError, match="format version 99"):
        ts.load(_trainer(), "models/2")
    open(meta_path, "w").write(json.dumps(meta))
    sr = _trainer(stochastic_rounding=True, sr_seed=7)
    _advance(sr, 4)
    ts.save(sr)
    with pytest.raises(ValueError, match="sr_seed 7"):
        ts.load(_trainer(stochastic_rounding=True, sr_seed=8), "models/4")
    # master weights: a param that is not bitwise bf16(master)
    m = _trainer(master_weights=True)
    _advance(m, 6)
    state = m.optimizer.state_dict()
    bad = dict(state, tensors=dict(state["tensors"], param=state["tensors"]["param"].clone()))
    bad["tensors"]["param"][3] += 1.0
    with pytest.raises(ValueError, match=r"not bitwise bf16\(master\)"):
        _trainer(master_weights=True).optimizer.load_state_dict(bad)
    _trainer(master_weights=True).optimizer.load_state_dict(state)
    # the sharded optimizer step
    m.model.shard = types.SimpleNamespace(rank=0, world=2, ddp=None)
    with pytest.raises(NotImplementedError, match="sharded"):
        m.optimizer.state_dict()
    with pytest.raises(NotImplementedError, match="sharded"):
        m.optimizer.load_state_dict(state)
