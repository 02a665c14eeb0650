"""The resumable state of a training run: ``models/<step>/trainer_state/`` (config keys ``save_state``, ``save_state_keep``,
``resume_from``; an extension of this package -- the reference saves the model only and cannot continue a run).

Bar: stop + resume = the uninterrupted run, on bits.  The state is captured after ``validate()`` and ``save_model()`` of step K
have returned and the EMA swap is undone -- the point from which the uninterrupted run goes on to step K + 1 -- and holds

* ``optimizer.safetensors``: ``FlatAdamW.state_dict()``'s tensors (the trained flat buffer, both moments, the EMA shadow and the
  fp32 master weights where present), written by rank 0 (the replicated step keeps them identical on every rank);
* ``rng_rank<r>.safetensors``: torch's CPU generator state, the device generator state and the sampler's device generator;
* ``rank<r>.json``: Python's ``random.getstate()`` and the sampler state of rank r, folded into
* ``state.json``, written LAST and by rename: format version, ``global_step``, the accumulation micro-step, the warm-up
  scheduler's ``last_epoch``, the world size, the optimizer's scalars with the layout fingerprint, the per-tensor device
  fingerprints (``ops.fingerprint``, include/yat_hip.h yat_fingerprint_u64) and the per-rank entries.  A directory without it
  is not a state: ``latest`` skips it and naming it is an error, so a killed save never leaves something that loads.

No pickle anywhere: tensors travel as safetensors, everything else as JSON, and the loader refuses a file that is a zip or a
pickle before handing it to any reader -- loading a state cannot run code.
"""
from __future__ import annotations

import json
import os
import random
import shutil
import time

import torch

FORMAT_VERSION = 1
DIR_NAME = "trainer_state"
_M64 = (1 << 64) - 1


def fingerprint_host(t, word_offset=0):
    """yat_fingerprint_u64 restated for a host tensor (numpy uint64): what ``fingerprint`` uses for a tensor that is not on a
    device, and the way to check a saved file without a GPU."""
    import numpy as np
    raw = t.detach().contiguous().view(torch.uint8).numpy().tobytes()
    if len(raw) == 0 or len(raw) % 4:
        raise ValueError(f"fingerprint: {len(raw)} bytes is not a positive multiple of 4")
    w = np.frombuffer(raw, dtype="<u4").astype(np.uint64)
    total = 0
    with np.errstate(over="ignore"):
        for lo in range(0, w.size, 1 << 22):
            part = w[lo:lo + (1 << 22)]
            g = np.arange(lo, lo + part.size, dtype=np.uint64) + np.uint64(int(word_offset) & _M64)
            z = ((g << np.uint64(32)) ^ (g >> np.uint64(32)) ^ part) + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z ^= z >> np.uint64(31)
            total = (total + int(z.sum(dtype=np.uint64))) & _M64
    return total


def fingerprint(t):
    """The 64-bit fingerprint of a flat buffer where it lives: the HIP kernel on a device, the restatement on the host."""
    if t.is_cuda:
        from .. import ops
        return ops.fingerprint(t)
    return fingerprint_host(t)


# ---------------------------------------------------------------------------------------------- directories
def state_dir(model_dir):
    return os.path.join(model_dir, DIR_NAME)


def is_complete(model_dir):
    return os.path.isfile(os.path.join(state_dir(model_dir), "state.json"))


def _steps(root):
    if not os.path.isdir(root):
        return []
    return sorted(int(n) for n in os.listdir(root) if n.isdigit() and os.path.isdir(os.path.join(root, n)))


def find_latest(root="models"):
    """The highest-numbered ``<root>/<step>`` with a complete state, or None."""
    for step in reversed(_steps(root)):
        if is_complete(os.path.join(root, str(step))):
            return os.path.join(root, str(step))
    return None


def resolve(resume_from, root="models"):
    """``latest`` -> ``find_latest`` (None: a fresh start); a directory named explicitly must hold a complete state."""
    if str(resume_from).strip().lower() == "latest":
        return find_latest(root)
    if not is_complete(resume_from):
        raise ValueError(f"resume_from: {resume_from} holds no complete trainer state ({DIR_NAME}/state.json is missing: the "
                         "save was not finished, or save_state was off)")
    return resume_from


def prune(keep, root="models"):
    """Keep the newest ``keep`` state directories under ``root`` and delete the older ones -- the state only: the model files
    of every step stay."""
    held = [s for s in _steps(root) if os.path.isdir(state_dir(os.path.join(root, str(s))))]
    removed = []
    for step in held[:max(0, len(held) - max(1, int(keep)))]:
        shutil.rmtree(state_dir(os.path.join(root, str(step))))
        removed.append(step)
    return removed


# ---------------------------------------------------------------------------------------------- files
def _write_json(path, obj):
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump(obj, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def _save_tensors(path, tensors):
    from safetensors.torch import save_file
    tmp = path + ".tmp"
    save_file({k: v.detach().cpu().contiguous() for k, v in tensors.items()}, tmp)
    os.replace(tmp, path)


def check_not_pickle(path):
    """A state file is JSON (its first byte opens an object) or safetensors (an 8-byte little-endian header length that fits
    the file, then a JSON object).  Anything else -- a zip archive (torch.save's container), a bare pickle, a gzip stream -- is
    refused before any reader sees the file."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(9)
    if path.endswith(".json"):
        ok = head[:1] == b"{"
    else:
        ok = len(head) == 9 and int.from_bytes(head[:8], "little") <= size - 8 and head[8:9] == b"{"
    if not ok:
        raise ValueError(f"{path}: a zip / pickle or otherwise foreign file, not a trainer state file (states hold safetensors "
                         "and JSON only)")


def _load_tensors(path):
    from safetensors.torch import load_file
    check_not_pickle(path)
    return load_file(path, device="cpu")


def _load_json(path):
    check_not_pickle(path)
    with open(path) as f:
        return json.load(f)


def _py_rng_to_json(st):
    return [st[0], list(st[1]), st[2]]


def _py_rng_from_json(st):
    return (int(st[0]), tuple(int(x) for x in st[1]), st[2])


# ---------------------------------------------------------------------------------------------- save
def save(trainer, model_dir=None):
    """Every rank calls this at the same point.  -> timings {fingerprint_s, d2h_s, write_s, total_s} on rank 0 (None elsewhere)."""
    acc, opt = trainer.accelerator, trainer.optimizer
    model_dir = model_dir or os.path.join("models", str(trainer.global_step))
    sdir = state_dir(model_dir)
    rank, world = acc.process_index, acc.num_processes
    t0 = time.perf_counter()
    state = opt.state_dict()                                  # (joins the overlapped update; refuses the sharded step)
    os.makedirs(sdir, exist_ok=True)
    stale = os.path.join(sdir, "state.json")
    if acc.is_main_process and os.path.exists(stale):
        os.remove(stale)                                      # a state being rewritten is not a state until it is whole again
    rng = {"torch_cpu": torch.get_rng_state()}
    if acc.device.type == "cuda":
        rng["torch_device"] = torch.cuda.get_rng_state(acc.device)
    sampler_state = trainer.sampler.state_dict() if trainer.sampler is not None else None
    if sampler_state is not None and sampler_state.get("generator") is not None:
        rng["sampler_device"] = torch.tensor(list(bytes.fromhex(sampler_state.pop("generator"))), dtype=torch.uint8)
        sampler_state["generator"] = "rng_file"
    _save_tensors(os.path.join(sdir, f"rng_rank{rank}.safetensors"), rng)
    _write_json(os.path.join(sdir, f"rank{rank}.json"), dict(python_random=_py_rng_to_json(random.getstate()), sampler=sampler_state))
    times = None
    if acc.is_main_process:
        t1 = time.perf_counter()
        prints = {k: f"{fingerprint(v):016x}" for k, v in state["tensors"].items()}
        t2 = time.perf_counter()
        host = {k: v.detach().cpu() for k, v in state["tensors"].items()}
        t2b = time.perf_counter()
        _save_tensors(os.path.join(sdir, "optimizer.safetensors"), host)
        del host
        t3 = time.perf_counter()
    acc.wait_for_everyone()                                   # every rank's entries are on disk
    if acc.is_main_process:
        sched = trainer.lr_scheduler
        meta = dict(format_version=FORMAT_VERSION, global_step=int(trainer.global_step), micro_step=int(acc._micro),
                    scheduler_last_epoch=None if sched is None else int(sched.last_epoch), world_size=world,
                    optimizer=state["scalars"], layout=state["layout"], fingerprints=prints,
                    ranks={str(r): _load_json(os.path.join(sdir, f"rank{r}.json")) for r in range(world)})
        _write_json(os.path.join(sdir, "state.json"), meta)   # last, by rename
        removed = prune(getattr(trainer.params, "save_state_keep", 1), os.path.dirname(os.path.abspath(model_dir)))
        t4 = time.perf_counter()
        times = dict(fingerprint_s=t2 - t1, d2h_s=t2b - t2, write_s=t3 - t2b, total_s=t4 - t0)
        print(f"trainer state: step {trainer.global_step} -> {sdir} (param fingerprint {prints['param']}, {t4 - t0:.2f} s"
              + (f", pruned {removed}" if removed else "") + ")")
        logger = getattr(trainer, "logger", None)
        if logger is not None:
            logger.add_scalar("train/param_fingerprint", int(prints["param"], 16) & 0xFFFFFFFF, trainer.global_step)
    acc.wait_for_everyone()
    return times


# ---------------------------------------------------------------------------------------------- load
def load(trainer, model_dir):
    """After ``initialize()`` has built optimizer, scheduler and sampler (and ``accelerator.prepare`` has run).  The trainer
    continues with step K + 1; the validate / save of K is not repeated and the restored master weights are the truth
    (``resync_master`` is not called).  -> timings {h2d_s, fingerprint_s, total_s}."""
    acc, opt = trainer.accelerator, trainer.optimizer
    if not is_complete(model_dir):
        raise ValueError(f"{model_dir} holds no complete trainer state ({DIR_NAME}/state.json is missing)")
    sdir = state_dir(model_dir)
    t0 = time.perf_counter()
    meta = _load_json(os.path.join(sdir, "state.json"))
    if meta.get("format_version") != FORMAT_VERSION:
        raise ValueError(f"{sdir}: format version {meta.get('format_version')}, this build reads {FORMAT_VERSION}")
    if int(meta["world_size"]) != acc.num_processes:
        raise ValueError(f"{sdir}: saved by {meta['world_size']} process(es), this job has {acc.num_processes}; resuming across a "
                         "different world size is not built")
    mine = meta["ranks"][str(acc.process_index)]
    tensors = _load_tensors(os.path.join(sdir, "optimizer.safetensors"))
    t1 = time.perf_counter()
    opt.load_state_dict(dict(tensors=tensors, scalars=meta["optimizer"], layout=meta.get("layout")))
    if acc.device.type == "cuda":
        torch.cuda.synchronize(acc.device)
    t2 = time.perf_counter()
    for name, t in opt._state_tensors().items():              # what sits in device memory now is what sat there at the save
        got, want = f"{fingerprint(t):016x}", meta["fingerprints"].get(name)
        if got != want:
            raise ValueError(f"{sdir}: tensor {name!r} of optimizer.safetensors has fingerprint {got}, the state recorded {want}: "
                             "the file was damaged or altered")
    t3 = time.perf_counter()
    if trainer.lr_scheduler is not None:
        if meta["scheduler_last_epoch"] is None:
            raise ValueError(f"{sdir}: saved without warmup_steps, this run has a warm-up scheduler")
        trainer.lr_scheduler.last_epoch = int(meta["scheduler_last_epoch"])
    elif meta["scheduler_last_epoch"] is not None:
        raise ValueError(f"{sdir}: saved with a warm-up scheduler, this run has none")
    acc._micro = int(meta["micro_step"])
    rng = _load_tensors(os.path.join(sdir, f"rng_rank{acc.process_index}.safetensors"))
    if trainer.sampler is not None and mine.get("sampler") is not None:
        sampler_state = dict(mine["sampler"])
        if sampler_state.get("generator") == "rng_file":
            sampler_state["generator"] = bytes(rng["sampler_device"].tolist()).hex()
        trainer.sampler.load_state_dict(sampler_state)
    random.setstate(_py_rng_from_json(mine["python_random"]))
    torch.set_rng_state(rng["torch_cpu"])
    if acc.device.type == "cuda" and "torch_device" in rng:
        torch.cuda.set_rng_state(rng["torch_device"], acc.device)
    trainer.global_step = int(meta["global_step"]) + 1
    t4 = time.perf_counter()
    print(f"trainer state: resumed from {sdir}: step {meta['global_step']} done, continuing at {trainer.global_step} "
          f"(param fingerprint {meta['fingerprints']['param']}, {t4 - t0:.2f} s)")
    return dict(read_s=t1 - t0, h2d_s=t2 - t1, fingerprint_s=t3 - t2, total_s=t4 - t0)
