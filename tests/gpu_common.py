"""What the VAE GPU test files share (test_dcae_gpu.py, test_dcae_encoder_gpu.py, test_vae_kl_gpu.py)."""
import os

import torch

BF = torch.bfloat16
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rbf(t):
    return t.to(BF).float()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()
