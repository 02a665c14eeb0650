"""What the GPU test files share: names and norms of the VAE files (test_dcae_gpu.py, test_dcae_encoder_gpu.py,
test_vae_kl_gpu.py), and the parity checks of the per-kernel files (test_kernels_gpu.py, test_rowops_gpu.py), whose
tolerances the docstring of test_kernels_gpu.py states.  A file that uses close() / as_good_as() imports the autouse
fixture _collect_failures into its own namespace."""
import os

import pytest
import torch

BF = torch.bfloat16
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rbf(t):
    return t.to(BF).float()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


_FAILS = []


@pytest.fixture(autouse=True)
def _collect_failures():
    _FAILS.clear()
    yield
    assert not _FAILS, "; ".join(_FAILS)


def close(a, b, name, tol=2e-3, ulps=2.0, atol=1e-6):
    a, b = a.float(), b.float()
    if not torch.isfinite(a).all():
        _FAILS.append(f"{name}: non-finite output")
        print(f"[parity] {name}: NON-FINITE")
        return
    r = rel(a, b)
    bound = ulps * 2.0 ** -8 * b.abs() + atol + 1e-3 * b.abs().mean()
    worst = ((a - b).abs() - bound).max().item()
    print(f"[parity] {name}: rel_l2={r:.3e} max_abs={(a - b).abs().max().item():.3e}")
    if r > tol:
        _FAILS.append(f"{name}: rel l2 {r:.3e} > {tol}")
    if worst > 0:
        _FAILS.append(f"{name}: element error exceeds {ulps} bf16 ulps by {worst:.3e}")


def as_good_as(hip, flow, truth, name, slack=1.25, floor=5e-4, tol_flow=6e-3):
    hip, flow, truth = hip.float(), flow.float(), truth.float()
    if not torch.isfinite(hip).all():
        _FAILS.append(f"{name}: non-finite output")
        print(f"[parity] {name}: NON-FINITE")
        return
    eh, ef, hf = rel(hip, truth), rel(flow, truth), rel(hip, flow)
    print(f"[parity] {name}: hip_vs_fp32={eh:.3e} torchbf16_vs_fp32={ef:.3e} hip_vs_torchbf16={hf:.3e}")
    if eh > slack * ef + floor:
        _FAILS.append(f"{name}: error vs fp32 truth {eh:.3e} > {slack} * reference's own {ef:.3e} + {floor}")
    if ef <= tol_flow and hf > tol_flow:      # (skipped when torch's own bf16 kernel is far from the truth)
        _FAILS.append(f"{name}: rel l2 vs torch bf16 flow {hf:.3e} > {tol_flow}")


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def rb(x):
    return x.to(BF).float()
