#!/usr/bin/env python3
"""Wall time of ONE trainer-state save and ONE restore (yat_amd/common/trainer_state.py) at SANA-1.6B's size, for each of the
three optimizer modes with the EMA shadow.

    python scripts/resume_state_times.py [--dir DIRECTORY] [--modes bf16,sr,master] [--out FILE.txt]

The state goes to a temporary directory (``--dir``, default: the system's) that is removed after every mode; a mode whose
state would not fit the free space twice over is reported as not measured.  Measured, no bar: the parts are the device
fingerprint of every tensor, the device->host copy, the safetensors write, and on the way back the read, the host->device copy
(with the master-weights mode's bf16(master) check on the host) and the fingerprints again."""
import argparse
import os
import shutil
import sys
import tempfile
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from yat_amd.common import trainer_state as ts  # noqa: E402
from yat_amd.common.trainer import HipAccelerator, WarmupLR  # noqa: E402
from yat_amd.optim import FlatAdamW  # noqa: E402
from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dir", default=None)
ap.add_argument("--modes", default="bf16,sr,master")
ap.add_argument("--layers", type=int, default=None, help="fewer layers than SANA-1.6B's (a rehearsal)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
os.environ["YAT_TENSORBOARD"] = "0"
cfg = SanaConfig() if a.layers is None else SanaConfig(num_layers=a.layers)
model = SanaTransformer2DModelHIP(cfg, device="cuda").init_synthetic(0)
lines = [f"device: {torch.cuda.get_device_name(0)}; SANA transformer of {model.numel_flat} parameters, use_ema, one process; "
         "one save and one restore per mode, host clock around work that ends in a device synchronise"]


def trainer(mode):
    t = types.SimpleNamespace()
    t.accelerator = HipAccelerator(1)
    t.model = model
    t.optimizer = FlatAdamW(model, lr=1e-5, use_ema=True, master_weights=mode == "master", stochastic_rounding=mode == "sr")
    t.lr_scheduler = WarmupLR(t.optimizer, 100)
    t.sampler, t.logger, t.global_step = None, None, 1000
    t.params = types.SimpleNamespace(save_state_keep=1)
    return t


for mode in a.modes.split(","):
    t = trainer(mode)
    opt = t.optimizer
    gen = torch.Generator(device="cuda").manual_seed(1)
    for buf in (opt.exp_avg, opt.exp_avg_sq):
        buf.copy_(torch.randn(buf.numel(), device="cuda", generator=gen, dtype=torch.bfloat16) * 1e-3)
    opt.step_count = opt.ema_steps = 1001
    nbytes = sum(v.numel() * v.element_size() for v in opt._state_tensors().values())
    root = tempfile.mkdtemp(prefix="yat_state_", dir=a.dir)
    try:
        free = shutil.disk_usage(root).free
        if free < 2 * nbytes:
            lines.append(f"{mode:6s} {nbytes / 1e9:6.2f} GB of tensors: not measured ({free / 1e9:.1f} GB free in {root})")
            continue
        torch.cuda.synchronize()
        s = ts.save(t, os.path.join(root, "models", "1000"))
        fresh = trainer(mode)
        for buf in fresh.optimizer._state_tensors().values():
            if buf is not model.flat_param:
                buf.zero_()
        torch.cuda.synchronize()
        r = ts.load(fresh, os.path.join(root, "models", "1000"))
        for k, v in opt._state_tensors().items():
            assert torch.equal(v, fresh.optimizer._state_tensors()[k]), k
        parts_s = {"fingerprint": s["fingerprint_s"], "D2H": s["d2h_s"], "file write": s["write_s"]}
        # (safetensors maps the file: the bytes are read from disk while they are checked and copied to the device)
        parts_r = {"file open": r["read_s"], "file read + checks + H2D": r["h2d_s"], "fingerprint": r["fingerprint_s"]}
        lines.append(f"{mode:6s} {nbytes / 1e9:6.2f} GB of tensors: save {s['total_s']:7.2f} s ("
                     + ", ".join(f"{k} {v:.3f}" for k, v in parts_s.items()) + f"; {max(parts_s, key=parts_s.get)} dominates); restore "
                     f"{r['total_s']:7.2f} s (" + ", ".join(f"{k} {v:.3f}" for k, v in parts_r.items())
                     + f"; {max(parts_r, key=parts_r.get)} dominates)")
        del fresh
    finally:
        shutil.rmtree(root, ignore_errors=True)
    del t, opt
    torch.cuda.empty_cache()
print("\n".join(lines))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
