"""Torch-CPU restatement of peft's FourierFT layer (test-only) and of the two-stage arithmetic of yat_amd/fourierft.py.

[RECALL peft/tuners/fourierft/layer.py -- peft is absent from this container: PARITY UNPINNED]  For a target Linear / 1x1 Conv
with weight [out, in] (the reference's call at common/trainer.py:231-237: alpha, scaling=1.0, ifft2_norm='ortho',
init_weights=True):
    idx = torch.randperm(out * in, generator=torch.Generator().manual_seed(random_loc_seed))[:n]; (u, v) = (idx // in, idx % in)
    dense[u, v] = fourierft_spectrum;  delta_w = torch.fft.ifft2(dense, norm=ifft2_norm).real * scaling
    result = base(x) + F.linear(x, delta_w)

* ``delta_f64`` / ``dc_f64``: the definition in float64 and autograd through it -- the truth.
* ``two_stage_delta`` / ``two_stage_dc``: the same values with the roundings of the HIP path -- the table in fp32, the scaled
  coefficient s * c one fp32 product, Y (Z) and the cos | -sin matrix B rounded to bf16, fp32 products and sums, one bf16 rounding
  of the result.  The order of the fp32 sums is torch's, not the kernels': bitwise agreement holds where the sums are exact or
  have at most two nonzero terms.
* ``apply_fourierft``: the wrap of an oracle model; the transform runs in fp32 (torch has no bf16 ifft2) and delta_w is cast to
  the module dtype.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.lokr_ref import is_target

BF = torch.bfloat16


def positions(out_dim, in_dim, n, seed=777):
    idx = torch.randperm(out_dim * in_dim, generator=torch.Generator().manual_seed(seed))[:n]
    return idx // in_dim, idx % in_dim


def norm_scale(norm, out_dim, in_dim, scaling=1.0):
    return scaling * {"backward": 1.0 / (out_dim * in_dim), "ortho": 1.0 / math.sqrt(out_dim * in_dim), "forward": 1.0}[norm]


def delta_from(c, u, v, out_dim, in_dim, norm="ortho", scaling=1.0):
    """ifft2(dense_spectrum, norm).real * scaling in c's (floating) dtype; differentiable in c."""
    dense = torch.zeros(out_dim, in_dim, dtype=c.dtype).index_put((u, v), c)
    return torch.fft.ifft2(dense, norm=norm).real * scaling


def delta_f64(c, u, v, out_dim, in_dim, norm="ortho", scaling=1.0):
    return delta_from(c.double(), u, v, out_dim, in_dim, norm, scaling)


def dc_f64(dd, u, v, out_dim, in_dim, norm="ortho", scaling=1.0):
    """d_spectrum for d_delta_w = dd by autograd through the float64 definition."""
    c = torch.zeros(u.numel(), dtype=torch.float64, requires_grad=True)
    (delta_from(c, u, v, out_dim, in_dim, norm, scaling) * dd.double()).sum().backward()
    return c.grad


def table_f64(d):
    m = torch.arange(d, dtype=torch.float64)
    return torch.stack([torch.cos(2 * math.pi * m / d), torch.sin(2 * math.pi * m / d)], 1)


def _oriented(u, v, out_dim, in_dim):
    """(short-dimension frequency, long-dimension frequency, rows, cols): out > in works on the transpose."""
    return (u, v, out_dim, in_dim) if out_dim <= in_dim else (v, u, in_dim, out_dim)


def _b_matrix(table_rows):
    d = table_rows.shape[0]
    j = torch.arange(d)
    idx = (j[:, None] * j[None, :]) % d
    return torch.cat([table_rows[idx, 0], -table_rows[idx, 1]], 1).to(BF).float()


def two_stage_delta(c, u, v, out_dim, in_dim, norm, scaling, table_rows, table_cols):
    """delta_w (bf16 [out, in]) from the bf16 spectrum c with the HIP path's roundings; the fp32 tables are the caller's (the
    product's ``twiddle_table``)."""
    a, b, rows, cols = _oriented(u, v, out_dim, in_dim)
    s = torch.tensor(norm_scale(norm, out_dim, in_dim, scaling), dtype=torch.float32)
    k = torch.arange(cols)
    y = torch.zeros(2 * rows, cols, dtype=torch.float32)
    for l in torch.sort(a, stable=True).indices.tolist():           # CSR order: by row, then by coefficient index
        w = table_cols[(int(b[l]) * k) % cols]
        sc = s * c[l].float()
        y[a[l]] += sc * w[:, 0]
        y[rows + a[l]] += sc * w[:, 1]
    d = _b_matrix(table_rows) @ y.to(BF).float()                    # [rows, cols]
    return (d if out_dim <= in_dim else d.t()).to(BF).contiguous()


def two_stage_dc(dd, u, v, out_dim, in_dim, norm, scaling, table_rows, table_cols):
    """d_spectrum (bf16 [n]) from the bf16 d_delta_w with the HIP path's roundings."""
    a, b, rows, cols = _oriented(u, v, out_dim, in_dim)
    s = torch.tensor(norm_scale(norm, out_dim, in_dim, scaling), dtype=torch.float32)
    g = dd.float() if out_dim <= in_dim else dd.float().t()
    z = (_b_matrix(table_rows).t() @ g).to(BF).float()              # [2 rows, cols]
    k = torch.arange(cols)
    out = torch.zeros(u.numel(), dtype=torch.float32)
    for l in range(u.numel()):
        w = table_cols[(int(b[l]) * k) % cols]
        out[l] = s * (z[a[l]] * w[:, 0] + z[rows + a[l]] * w[:, 1]).sum()
    return out.to(BF)


class FourierFTWrapped(nn.Module):
    def __init__(self, base, n_frequency, scaling=1.0, norm="ortho", random_loc_seed=777):
        super().__init__()
        self.base_layer = base
        for p in base.parameters():
            p.requires_grad_(False)
        if isinstance(base, nn.Conv2d):
            assert base.kernel_size == (1, 1), "only 1x1 convolutions are targeted here"
            self.out_dim, self.in_dim = base.out_channels, base.in_channels
        else:
            self.out_dim, self.in_dim = base.out_features, base.in_features
        self.scaling, self.norm = scaling, norm
        u, v = positions(self.out_dim, self.in_dim, n_frequency, random_loc_seed)
        self.register_buffer("u", u, persistent=False)
        self.register_buffer("v", v, persistent=False)
        self.fourierft_spectrum = nn.Parameter(torch.zeros(n_frequency, dtype=base.weight.dtype))      # init_weights=True

    def delta_weight(self):
        d = delta_from(self.fourierft_spectrum.float(), self.u, self.v, self.out_dim, self.in_dim, self.norm, self.scaling)
        return d.to(self.base_layer.weight.dtype).reshape(self.base_layer.weight.shape)

    def forward(self, x):
        dw = self.delta_weight()
        xin = x.to(dw.dtype)
        return self.base_layer(x) + (F.conv2d(xin, dw) if isinstance(self.base_layer, nn.Conv2d) else F.linear(xin, dw))


def apply_fourierft(model, targets, alpha=None, n_frequency=None, scaling=1.0, norm="ortho", random_loc_seed=777):
    """Wrap every target module in place (get_peft_model); freezes ALL base parameters.  Returns {dotted name: wrapper}."""
    assert (alpha is None) != (n_frequency is None)
    for p in model.parameters():
        p.requires_grad_(False)
    wrapped = {}
    for name, mod in list(model.named_modules()):
        if not isinstance(mod, (nn.Linear, nn.Conv2d)) or not is_target(name, targets):
            continue
        parent = model
        parts = name.split(".")
        for part in parts[:-1]:
            parent = parent[int(part)] if part.isdigit() else getattr(parent, part)
        out_dim, in_dim = mod.weight.shape[0], mod.weight.numel() // mod.weight.shape[0]
        n = n_frequency if alpha is None else max(1, int(alpha * out_dim * in_dim))
        w = FourierFTWrapped(mod, n, scaling, norm, random_loc_seed)
        if parts[-1].isdigit():
            parent[int(parts[-1])] = w
        else:
            setattr(parent, parts[-1], w)
        wrapped[name] = w
    return wrapped
