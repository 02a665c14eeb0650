"""FourierFT adapters on the HIP path (``lora_algo: fourierft`` -- the reference wraps the transformer with peft's
``FourierFTConfig(target_modules, init_weights=True, alpha=fourierft_alpha, scaling=1.0, ifft2_norm='ortho')`` at
common/trainer.py:231-237 and hands the spectra to AdamW).

Arithmetic [RECALL peft/tuners/fourierft/layer.py -- parity unpinned, see tests/fourierft_ref.py for the restatement]: for a
target Linear / 1x1 Conv with weight W [out, in]:
    idx = torch.randperm(out * in, generator=torch.Generator().manual_seed(random_loc_seed))[:n];  u = idx // in, v = idx % in
    dense_spectrum[u, v] = fourierft_spectrum  (n real coefficients, zeros at init; zero elsewhere)
    delta_w = ifft2(dense_spectrum, norm).real * scaling
            = s * sum_l c_l cos(2 pi (u_l j / out + v_l k / in)),   s = scaling * {1/(out in), 1/sqrt(out in), 1}[norm]
    result  = base_layer(x) + F.linear(x, delta_w)
with n = max(1, int(alpha * out * in)) per target when ``alpha`` is given (the reference's call) and ``n_frequency`` otherwise.
The positions are the same for every run (seed 777) and are never saved.  torch has no bf16 ``ifft2``, so the reference's own
bf16 branch cannot run; here the transform is computed in fp32 from the bf16 spectrum and delta_w is rounded to bf16 once.

MI355X mapping -- the *dense* application (``DenseDelta`` of yat_amd/adapters.py) with a sparse-spectrum inverse DFT as the
``delta_w`` builder.  The transform is separable: the LONG dimension runs sparsely (``yat_fourier_expand``: only the populated
positions cost, cos / sin from a host-built table), the SHORT one is a GEMM against a [rows, 2 rows] cos | -sin matrix on the
matrix cores.  With out > in the class works on the transpose: the positions are grouped by v, and the GEMM runs with a_t so
that delta_w still lands [out, in] row-major at the target weight's offset of the delta shadow.  ``project()`` is the adjoint:
Z = B^T d_delta_w (GEMM), then ``yat_fourier_contract``.  The spectra live in one flat bf16 buffer (n padded to 8 per target:
the padding is zero and stays zero), so clip + AdamW, master weights, stochastic rounding, the data-parallel all-reduce and the
resumable state are the usual launches.  There is no module dropout (peft's layer has none).
"""
from __future__ import annotations

import math

import torch

from . import ops
from .adapters import AdapterSet, DenseDelta

BF16 = torch.bfloat16
MAX_DIM = 46340                 # phases are (v * k) mod d in 32-bit integers
NORMS = ("backward", "ortho", "forward")


def twiddle_table(d: int) -> torch.Tensor:
    """T[m] = (cos, sin)(2 pi m / d), m < d, as fp32 pairs [d, 2], from doubles.  The angle is reduced to the first octant in
    integer arithmetic first (8 m = q d + r; an odd octant is walked backwards), so multiples of a quarter turn come out exactly
    0 or +-1 and T[d - m] is the conjugate of T[m] on bits.  Zeros are +0."""
    if not 1 <= d <= MAX_DIM:
        raise ValueError(f"twiddle table: dimension {d} is outside 1..{MAX_DIM}")
    m = torch.arange(d, dtype=torch.int64)
    q, r = torch.div(8 * m, d, rounding_mode="floor"), (8 * m) % d
    r = torch.where(q % 2 == 1, d - r, r)
    ang = math.pi * r.to(torch.float64) / (4.0 * d)             # in [0, pi / 4]
    c, s = torch.cos(ang), torch.sin(ang)
    pick = lambda octants: torch.stack(octants)[q, m] + 0.0
    cos, sin = pick([c, s, -s, -c, -c, -s, s, c]), pick([s, c, c, s, -s, -c, -c, -s])
    return torch.stack([cos, sin], dim=1).to(torch.float32)


def positions(out_dim: int, in_dim: int, n: int, seed: int = 777):
    """The n populated positions (u, v) of the [out, in] spectrum, in the order of the coefficients (peft's draw, on the CPU)."""
    if not 1 <= n <= out_dim * in_dim:
        raise ValueError(f"n_frequency {n} is outside 1..{out_dim * in_dim}")
    idx = torch.randperm(out_dim * in_dim, generator=torch.Generator().manual_seed(seed))[:n]
    return idx // in_dim, idx % in_dim


def n_from_alpha(alpha: float, out_dim: int, in_dim: int) -> int:
    return max(1, int(alpha * out_dim * in_dim))


def build_csr(u, v, out_dim: int, in_dim: int):
    """CSR over the SHORT dimension's frequencies: out <= in groups the positions by u (col = v), out > in by v (col = u).
    -> row_ptr [rows + 1], col [n], perm [n] (int32): entry e of the CSR is coefficient perm[e]; within a row the entries keep
    the coefficients' order."""
    key, other, rows = (u, v, out_dim) if out_dim <= in_dim else (v, u, in_dim)
    perm = torch.sort(key, stable=True).indices
    row_ptr = torch.zeros(rows + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(torch.bincount(key, minlength=rows), 0)
    return row_ptr.to(torch.int32), other[perm].to(torch.int32), perm.to(torch.int32)


def dft_matrix(table: torch.Tensor) -> torch.Tensor:
    """B [d, 2 d] bf16 from the table of d (on the table's device): B[j, u] = cos 2 pi (u j mod d) / d, B[j, d + u] = -sin .."""
    d = table.shape[0]
    j = torch.arange(d, device=table.device)
    idx = (j[:, None] * j[None, :]) % d
    return torch.cat([table[idx, 0], -table[idx, 1]], dim=1).to(BF16)


def norm_factor(norm: str, out_dim: int, in_dim: int) -> float:
    return {"backward": 1.0 / (out_dim * in_dim), "ortho": 1.0 / math.sqrt(out_dim * in_dim), "forward": 1.0}[norm]


def expand_gemm(spectrum, s, out_dim, in_dim, csr, table, B, y, d):
    """d [out, in] <- delta_w of one target: ``spectrum`` (at least n bf16 coefficients), ``csr`` of ``build_csr`` on the device,
    ``table`` of the long dimension, ``B`` of the short one, ``y`` a [2 rows, cols] scratch view; y and d may have row strides."""
    rows = min(out_dim, in_dim)
    ops.fourier_expand(*csr, spectrum, s, table, y)
    if out_dim <= in_dim:                                                                  # delta_w = B Y
        ops.gemm(B, y, d, b_t=True, M=out_dim, N=in_dim, K=2 * rows, lda=2 * rows, ldb=y.stride(0), ldc=d.stride(0))
    else:                                                                                  # delta_w = Y^T B^T
        ops.gemm(y, B, d, a_t=True, M=out_dim, N=in_dim, K=2 * rows, lda=y.stride(0), ldb=2 * rows, ldc=d.stride(0))


def gemm_contract(dd, s, out_dim, in_dim, csr, table, B, z, g):
    """g[:n] <- d_spectrum of one target from dd = d_delta_w [out, in]: the adjoint of ``expand_gemm`` (z: a [2 rows, cols]
    scratch view)."""
    rows, cols = min(out_dim, in_dim), max(out_dim, in_dim)
    # Z = B^T d_delta_w (out <= in), Z = B^T d_delta_w^T (out > in: dd is the [N, K] operand)
    ops.gemm(B, dd, z, a_t=True, b_t=out_dim <= in_dim, M=2 * rows, N=cols, K=rows, lda=2 * rows, ldb=dd.stride(0),
             ldc=z.stride(0))
    ops.fourier_contract(*csr, z, s, table, g)


class FourierFTAdapters(DenseDelta, AdapterSet):
    kind, refuses_conv = "FourierFT", ""

    def __init__(self, model, targets, n_frequency=None, alpha=None, scaling: float = 1.0, norm: str = "ortho",
                 random_loc_seed: int = 777):
        if (n_frequency is None) == (alpha is None):
            raise ValueError("FourierFT: give exactly one of n_frequency and alpha")
        if norm not in NORMS:
            raise ValueError(f"FourierFT: ifft2_norm {norm!r} is not one of {NORMS}")
        self.n_frequency = None if n_frequency is None else int(n_frequency)
        self.alpha = None if alpha is None else float(alpha)
        self.scale, self.norm, self.random_loc_seed = float(scaling), norm, int(random_loc_seed)
        self._scan(model, targets)
        dev = model.flat_param.device
        # one CSR per distinct (out, in, n) -- the same seed gives the same positions --, one table per dimension, one B per
        # short dimension, one Y / Z scratch for the largest target
        self._csr, self._table, self._B = {}, {}, {}
        for e in self.entries:
            out, inn, n = e["out"], e["inn"], e["n"]
            rows, cols = min(out, inn), max(out, inn)
            if (out, inn, n) not in self._csr:
                u, v = positions(out, inn, n, self.random_loc_seed)
                self._csr[(out, inn, n)] = tuple(t.to(dev) for t in build_csr(u, v, out, inn))
            for d in (rows, cols):
                if d not in self._table:
                    self._table[d] = twiddle_table(d).to(dev)
            if rows not in self._B:
                self._B[rows] = dft_matrix(self._table[rows])
        self.delta = torch.zeros_like(model.flat_param)
        self._yz = torch.empty(max(2 * e["out"] * e["inn"] for e in self.entries), dtype=BF16, device=dev)
        self._attach()

    def _n_for(self, out_dim, in_dim):
        return n_from_alpha(self.alpha, out_dim, in_dim) if self.alpha is not None else self.n_frequency

    def _lay_out(self, key, w, out_dim, in_dim, off):
        """fourierft_spectrum [n], padded to a multiple of 8"""
        n = self._n_for(out_dim, in_dim)
        if not 1 <= n <= out_dim * in_dim:
            raise ValueError(f"{key}: n_frequency {n} is outside 1..{out_dim * in_dim}")
        if max(out_dim, in_dim) > MAX_DIM:
            raise NotImplementedError(f"{key}: FourierFT on a layer wider than {MAX_DIM} is not built (32-bit phases)")
        return dict(o=off, n=n, has_grad=False), [off + (n + 7) // 8 * 8]

    def _views(self, e, flat):
        """The target's coefficients and its whole padded segment."""
        return flat[e["o"]:e["o"] + e["n"]], flat[e["o"]:e["o"] + (e["n"] + 7) // 8 * 8]

    def _s(self, e):
        return self.scale * norm_factor(self.norm, e["out"], e["inn"])

    def reset_parameters(self):
        """peft init_weights=True: the spectrum is zeros."""
        self.flat_param.zero_()

    def _plan(self, e):
        out, inn = e["out"], e["inn"]
        rows, cols = min(out, inn), max(out, inn)
        return self._csr[(out, inn, e["n"])], self._table[cols], self._B[rows], self._yz[:2 * rows * cols].view(2 * rows, cols)

    # ---- per step
    def materialize(self, training=True):
        self.join_pending_update()
        first_micro = not getattr(self.model, "accumulate_grads", False)
        for e in self.entries:
            if first_micro:
                e["has_grad"] = False       # a new accumulation window: nothing has contributed yet
            csr, table, B, y = self._plan(e)
            expand_gemm(self._views(e, self.flat_param)[1], self._s(e), e["out"], e["inn"], csr, table, B, y,
                        self._shadow(e, self.delta))

    def wgrad(self, dy, x, gw, accumulate=False, hs=None):
        """d_delta_w of the target(s) behind ``gw`` into their flat-gradient slots (the base weights are frozen)."""
        for e, row0 in self.lookup(gw, self.model.flat_grad):
            self._dense_wgrad(e, dy[:, row0:row0 + e["out"]], x, accumulate)

    def project(self):
        """d_delta_w -> d_spectrum: the adjoint of ``materialize``."""
        for e in self.entries:
            g = self._views(e, self.flat_grad)[1]
            if not e["has_grad"]:
                g.zero_()
                continue
            csr, table, B, z = self._plan(e)
            gemm_contract(self._shadow(e, self.model.flat_grad), self._s(e), e["out"], e["inn"], csr, table, B, z, g)
        super().project()

    # ---- checkpoint (peft layout)
    def state_dict(self):
        self.join_pending_update()
        return {self._peft_prefix(e) + "fourierft_spectrum": self._views(e, self.flat_param)[0].clone() for e in self.entries}

    def load_state_dict(self, sd):
        for e in self.entries:
            c = self._views(e, self.flat_param)[0]
            t = sd[self._peft_prefix(e) + "fourierft_spectrum"]
            if t.numel() != e["n"]:
                raise ValueError(f"{e['module']}: the saved spectrum has {t.numel()} coefficients, this adapter {e['n']}")
            c.copy_(t.to(device=c.device, dtype=BF16).reshape(-1))

    def _peft_config(self):
        return {"peft_type": "FOURIERFT", "n_frequency": self.n_frequency if self.n_frequency is not None else 1000,
                "alpha": self.alpha, "n_frequency_pattern": {e["module"]: e["n"] for e in self.entries}, "scaling": self.scale,
                "random_loc_seed": self.random_loc_seed, "ifft2_norm": self.norm, "init_weights": True,
                "target_modules": self.targets}

    @classmethod
    def from_peft_config(cls, model, conf):
        """The adapter set a saved ``adapter_config.json`` describes (``lora_pretrained``)."""
        kw = dict(alpha=conf["alpha"]) if conf.get("alpha") is not None else dict(n_frequency=int(conf["n_frequency"]))
        return cls(model, conf["target_modules"], scaling=float(conf.get("scaling", 1.0)), norm=conf.get("ifft2_norm", "ortho"),
                   random_loc_seed=int(conf.get("random_loc_seed", 777)), **kw)

    def num_parameters(self):
        return sum(e["n"] for e in self.entries)
