"""`python bench.py --gpus N` must start by itself (round-3 review, item 1): with N > 1 and no launcher around it the parent
starts `python -m torch.distributed.run` as a fresh child process before anything touches the GPU, relays rank 0's one JSON
line and the exit code.  The reference's counterpart is `accelerate launch` (README.md:62, common/trainer.py:31-37)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def test_self_launch_starts_ranks_and_relays_exit_code():
    """No GPU here: both ranks the parent started must say so and the parent must hand their failure back."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-side check of the launcher (the GPU box runs test_self_launch_world2_over_gloo_on_one_gpu)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--no-cpu-baseline"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "without a launcher: starting" in r.stderr                 # the parent took the self-launch path ...
    assert "--nproc-per-node=2" in r.stderr
    assert "bench.py needs a GPU" in r.stderr                          # ... and a rank ran bench.py's own main() (the launcher
    #                                                                    ends the other one as soon as the first has failed)
    assert r.stdout.strip() == ""                                      # no JSON line from a failed run


def test_world_size_mismatch_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=_env(WORLD_SIZE="2", RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "disagree" in r.stderr


@pytest.mark.gpu
def test_self_launch_world2_over_gloo_on_one_gpu():
    """The driver's N > 1 command shape, by itself: two ranks on cuda:0 (RCCL refuses two ranks on one device, so the
    transport is gloo; everything else -- rank discovery, broadcast, bucket hooks, barrier + max over ranks -- is the N > 1
    path), a 2-block model, the JSON line on stdout and nothing else."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--layers", "2", "--steps", "2",
                        "--warmup", "1", "--full", "--no-cpu-baseline", "--no-gemm-timer", "--comm-steps", "2"],
                       env=_env(YAT_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 16
    assert d["value"] > 0 and d["scaling"] == "weak"
    assert d["comm"]["world"] == 2 and "error" not in d["comm"]
    # what the communicator itself saw (round-4 review 5b), not the launcher's environment; and the channel cap in force
    assert d["comm"]["communicator"]["world"] == 2 and d["comm"]["communicator"]["rank"] == 0
    assert "gloo" in d["comm"]["communicator"]["owner"]
    assert d["comm"]["rccl_channels"]["NCCL_MAX_NCHANNELS"] is None          # RCCL's default unless asked (yat_amd/ddp.py)


def _plain_run(out, *args):
    """bench.py --gpus 1 --layers 2 ARGS --dump-outputs OUT -> (the JSON line, {name: array} of the dump)."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--layers", "2", *args,
                        "--dump-outputs", str(out)], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {p.stem: np.load(p) for p in sorted(out.glob("*.npy"))}


@pytest.mark.gpu
def test_plain_run_times_steps_and_dumps_outputs(tmp_path):
    """A plain run (no --full) times --steps steps, prints the contract keys and none of the side measurements, and
    --dump-outputs writes the last timed step's outputs as float32 .npy files (64 MB at most in all) -- the same ones
    again when the run is repeated with the same arguments."""
    import numpy as np
    d, arrays = _plain_run(tmp_path / "a", "--steps", "3", "--warmup", "1")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 8 * 3 / (3 * d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for side in ("roofline", "roofline_hbm", "cpu_baseline", "comm", "host_enqueue_ms_per_step"):
        assert side not in d, side
    assert set(arrays) == {"loss", "grad_norm", "params_sample", "grads_sample"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["params_sample"].shape == arrays["grads_sample"].shape and arrays["params_sample"].size > 1
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert np.isclose(arrays["loss"][0], d["loss"], rtol=1e-6) and arrays["grad_norm"][0] > 0
    assert np.count_nonzero(arrays["grads_sample"]) > arrays["grads_sample"].size // 2      # written by the backward
    _, again = _plain_run(tmp_path / "b", "--steps", "3", "--warmup", "1")
    for name, a in arrays.items():
        assert np.array_equal(a, again[name]), f"{name} differs between two runs with the same arguments"


@pytest.mark.gpu
def test_dumped_parameters_are_those_after_the_last_update(tmp_path):
    """One step from the seeded initial weights: AdamW's first update is -lr * g / (|g| + eps), so every sampled parameter
    that moved has moved against the sign of its dumped gradient, and some have moved (the dump is read after the
    optimizer stream's update, not before it)."""
    import numpy as np
    import torch
    import bench
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    _, arrays = _plain_run(tmp_path / "one", "--steps", "1", "--warmup", "0")
    model = SanaTransformer2DModelHIP(SanaConfig(num_layers=2), device="cuda:0").init_synthetic(seed=0)   # bench.py's weights
    idx = bench.dump_positions(model.numel_flat)
    p0 = (model.flat_param if idx is None else model.flat_param[idx.to(model.flat_param.device)]).float().cpu().numpy()
    del model
    torch.cuda.empty_cache()
    p1, g = arrays["params_sample"], arrays["grads_sample"]
    moved = p1 != p0
    assert moved.sum() > 1000, f"only {moved.sum()} of {p1.size} sampled parameters changed in the step"
    assert np.array_equal(np.sign(p1 - p0)[moved], -np.sign(g)[moved])
