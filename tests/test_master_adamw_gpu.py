"""``FlatAdamW(master_weights=True, use_ema=True)`` -- yat_adamw_master_step (csrc/optim.hip) -- against torch (GPU).

References, both on the CPU: ``torch.optim.AdamW`` + ``LambdaLR`` warm-up + ``oracle.recipe_ref.EMAModelRef`` on float32
parameters (the yardstick) and on float64 parameters (the truth).  The update is elementwise, so the references hold the flat
buffer as one parameter.  Both are fed the bf16 gradients converted to their dtype and multiplied by HIP's own clip
coefficient; that coefficient is asserted equal to torch's ``clip_grad_norm_`` arithmetic on HIP's norm (the norm itself is held
to torch by tests/test_optim_gpu.py, whose kernels this mode does not touch).

Bars, per step and per buffer (master, exp_avg, exp_avg_sq, EMA shadow):
    max|hip - f64| <= 2 max|f32 - f64|        and        ||hip - f64|| / ||f64|| <= 2 ||f32 - f64|| / ||f64||.
The factor 2: hipcc may contract a product into a sum with one rounding where torch's CPU build takes two, or the other way
round; an fp32 emulation of the kernel with every such product-sum fused sits at ratio 1.000 of torch's float32 error (max abs
error 8e-9 ... 4e-8, relative L2 3e-8 ... 1.7e-7), a wrong element at a vector edge is off by orders of magnitude more.  After
each step's comparison both CPU runs take HIP's fp32 state, so one step's rounding does not compound.

Exact, every step: the bf16 flat buffer is bitwise ``master.to(bfloat16)`` (NaN positions equal); a whole-buffer launch with
``zero_grad`` on a twin of the state gives the same bits as the optimizer's own launches and leaves the twin's gradients zero.

Inputs: weights N(0, 0.5^2) (small layouts) or N(0, 0.02^2) (grid wrap); gradient magnitudes log-uniform over 1e-8 ... 1 with
exact zeros, scaled per step so that the clip coefficient is below 1 in steps 1 and 3 and exactly 1 in steps 2 and 4; no
intermediate is subnormal.  Warm-up of 2: step 1 runs at lr 0, step 2 at lr / 2.
"""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernels_gpu import BF, DEV, ops  # noqa: F401  (fixture)
from test_optim_gpu import _same, _torch_coef, _up

pytestmark = pytest.mark.gpu

WARMUP, LR, EMA_DECAY = 2, 1e-3, 0.999
CLIPPED = (True, False, True, False)          # per step: gradient norm far above 1, then below 1
BUFFERS = ("master", "exp_avg", "exp_avg_sq", "ema_shadow")
SMALL_SHAPES = [(96, 40), (40,), (3, 3, 16), (2000,), (8,)]      # the layout of test_nonfinite_gradient_follows_torch
SMALL_BUCKETS = [[0, 1], [2, 3, 4]]


# ------------------------------------------------------------------------------------------------ helpers
def _layout(shapes, buckets):
    starts, lows, off = [], [], 0
    for b in buckets:
        off = _up(off, 64)
        lows.append(off)
        for t in b:
            starts.append(off)
            off += _up(math.prod(shapes[t]), 8)
    off = _up(off, 64)
    return starts, list(zip(lows, lows[1:] + [off])), off


def _stand_in(starts, bounds, n, weight_std, seed, **extra):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    flat = (torch.randn(n, generator=gen, device=DEV) * weight_std).to(BF)
    return SimpleNamespace(flat_param=flat, flat_grad=torch.zeros(n, dtype=BF, device=DEV),
                           seg_start=torch.tensor(starts + [n], dtype=torch.int64), numel_flat=n, bucket_bounds=bounds,
                           param_events=None, join_pending_update=torch.cuda.synchronize, **extra)


def _fill_grad(model, seed, scale):
    """|g| = scale * 10^U(-8, 0), random sign, one element in 16 exactly zero; rounded to bf16 on the device."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n = model.numel_flat
    mag = torch.pow(10.0, torch.rand(n, generator=gen, device=DEV) * -8.0) * scale
    sign = torch.where(torch.rand(n, generator=gen, device=DEV) < 0.5, -1.0, 1.0)
    keep = torch.rand(n, generator=gen, device=DEV) >= 1.0 / 16
    model.flat_grad.copy_((mag * sign * keep).to(BF))


def _grad_scale(n, clipped):
    """E[g^2] of the log-uniform draw is 1 / (16 ln 10) ~ 0.165^2: a norm of ~0.165 sqrt(n) at scale 1, ~0.25 when not clipped."""
    return 1.0 if clipped else 0.25 / (0.165 * math.sqrt(n))


class _Ref:
    """torch.optim.AdamW + LambdaLR warm-up + EMAModelRef on ONE flat CPU parameter of ``dtype``."""

    def __init__(self, flat_bf16, dtype, lr, weight_decay, warmup=WARMUP):
        from oracle.recipe_ref import EMAModelRef
        self.dtype = dtype
        self.p = torch.nn.Parameter(flat_bf16.cpu().to(dtype))
        self.opt = torch.optim.AdamW([self.p], lr=lr, weight_decay=weight_decay)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.opt, lambda s: s / warmup if s < warmup else 1.0) if warmup else None
        self.ema = EMAModelRef([self.p], decay=EMA_DECAY)

    def step(self, grad_bf16_cpu, coef):
        g = grad_bf16_cpu.to(self.dtype)
        self.p.grad = g if coef is None else g * coef          # grads.mul_(clip_coef_clamped), exact in either dtype
        self.opt.step()
        if self.sched is not None:
            self.sched.step()
        self.ema.step([self.p])

    def buffers(self):
        st = self.opt.state[self.p]
        return {"master": self.p.data, "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"], "ema_shadow": self.ema.shadow_params[0]}

    def take(self, hip):
        for k, t in self.buffers().items():
            t.copy_(hip[k].to(self.dtype))


def _hip_buffers(opt):
    return {k: getattr(opt, k).cpu() for k in BUFFERS}


def _bars(hip, r32, r64, sl, name, worst):
    """The two bars on every buffer over the slice ``sl``; the measured ratios are printed and the largest kept in ``worst``."""
    b32, b64 = r32.buffers(), r64.buffers()
    for k in BUFFERS:
        h, a, t = hip[k][sl].double(), b32[k][sl].double(), b64[k][sl]
        assert torch.isfinite(t).all() and torch.isfinite(h).all(), f"{name} {k}: non-finite values"
        e_h, e_a = (h - t).abs().max().item(), (a - t).abs().max().item()
        l_h, l_a = ((h - t).norm() / t.norm()).item(), ((a - t).norm() / t.norm()).item()
        r_max = e_h / e_a if e_a else (0.0 if e_h == 0 else math.inf)
        r_l2 = l_h / l_a if l_a else (0.0 if l_h == 0 else math.inf)
        print(f"[master] {name} {k}: max abs error hip {e_h:.3e} f32 {e_a:.3e} (ratio {r_max:.3f}); "
              f"relative L2 hip {l_h:.3e} f32 {l_a:.3e} (ratio {r_l2:.3f})")
        worst["max"], worst["l2"] = max(worst["max"], r_max), max(worst["l2"], r_l2)
        assert e_h <= 2 * e_a, f"{name} {k}: max|hip - f64| {e_h:.3e} > 2 x {e_a:.3e}"
        assert l_h <= 2 * l_a, f"{name} {k}: relative L2 error {l_h:.3e} > 2 x {l_a:.3e}"


def _assert_working_copy(model, opt, name):
    """flat_param is bitwise bf16(master); NaN at the same positions."""
    want = opt.master.to(BF)
    nan_w, nan_p = torch.isnan(want), torch.isnan(model.flat_param)
    assert torch.equal(nan_w, nan_p), f"{name}: NaN positions of the bf16 copy differ from bf16(master)"
    assert torch.equal(model.flat_param[~nan_p].view(torch.int16), want[~nan_w].view(torch.int16)), f"{name}: flat_param is not bf16(master)"


def _check_coef(opt, max_grad_norm):
    total = torch.tensor(opt.grad_norm.item(), dtype=BF)
    assert _same(total.float().item(), opt.grad_norm.item())
    coef = opt.clip_coef.item()
    assert _same(_torch_coef(total, max_grad_norm), coef), f"clip coefficient {coef!r} against torch's on HIP's norm {total!r}"
    return coef


def _run_steps(ops, model, opt, weight_decay, max_grad_norm, name, sl=slice(None), twin=False, seed=100):
    """4 warm-up / full-rate steps of ``opt`` on ``model`` against the two CPU runs; returns the clip coefficients seen."""
    from yat_amd.common.trainer import WarmupLR
    r32 = _Ref(model.flat_param, torch.float32, LR, weight_decay)
    r64 = _Ref(model.flat_param, torch.float64, LR, weight_decay)
    sched = WarmupLR(opt, WARMUP)
    coefs, worst = [], {"max": 0.0, "l2": 0.0}
    for step, clipped in enumerate(CLIPPED, 1):
        _fill_grad(model, seed + step, _grad_scale(model.numel_flat, clipped))
        g_cpu = model.flat_grad.cpu()
        lr = opt.param_groups[0]["lr"]
        assert abs(lr - r32.opt.param_groups[0]["lr"]) <= 1e-18 and lr == (0.0, LR / 2, LR, LR)[step - 1]
        if twin:
            tw = {k: getattr(opt, k).clone() for k in BUFFERS}
            tw_p, tw_g = model.flat_param.clone(), model.flat_grad.clone()
        opt.step()
        sched.step()
        model.join_pending_update()
        torch.cuda.synchronize()
        coef = None
        if max_grad_norm is not None:
            coef = _check_coef(opt, max_grad_norm)
            coefs.append(coef)
            assert (coef < 1.0) == clipped
        _assert_working_copy(model, opt, f"{name} step {step}")
        if twin:
            # the same step as ONE launch over the whole buffer with the gradient clear: same bits, gradients zero
            ops.adamw_master_step(tw_p, tw["master"], tw_g, tw["exp_avg"], tw["exp_avg_sq"], None if coef is None else opt.clip_coef,
                                  lr, 0.9, 0.999, 1e-8, weight_decay, step, zero_grad=True, ema_shadow=tw["ema_shadow"],
                                  ema_decay=opt._ema_decay_now())
            torch.cuda.synchronize()
            assert not tw_g.view(torch.int16).any(), f"{name} step {step}: zero_grad left gradients"
            assert torch.equal(tw_p.view(torch.int16), model.flat_param.view(torch.int16))
            for k in BUFFERS:
                assert torch.equal(tw[k].view(torch.int32), getattr(opt, k).view(torch.int32)), f"{name} step {step}: {k} differs from the whole-buffer launch"
            assert torch.equal(model.flat_grad.cpu().view(torch.int16), g_cpu.view(torch.int16)), "the optimizer's own step cleared gradients"
        r32.step(g_cpu, coef)
        r64.step(g_cpu, coef)
        assert opt._ema_decay_now() == r32.ema.cur_decay_value
        hip = _hip_buffers(opt)
        _bars(hip, r32, r64, sl, f"{name} step {step}", worst)
        r32.take(hip)
        r64.take(hip)
    if max_grad_norm is not None:
        assert min(coefs) < 1.0 and max(coefs) == 1.0
    print(f"[master] {name}: largest ratio to torch float32's error: max abs {worst['max']:.3f}, relative L2 {worst['l2']:.3f}")
    return coefs


# ------------------------------------------------------------------------------------------------ a. small layouts
@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
@pytest.mark.parametrize("max_grad_norm", [1.0, None], ids=["clip", "no_clip"])
@pytest.mark.parametrize("weight_decay", [0.01, 0.0], ids=["wd", "no_wd"])
def test_master_step_small_layout(ops, weight_decay, max_grad_norm, overlap):
    from yat_amd.optim import FlatAdamW
    starts, bounds, n = _layout(SMALL_SHAPES, SMALL_BUCKETS)
    model = _stand_in(starts, bounds, n, 0.5, seed=23)
    opt = FlatAdamW(model, lr=LR, weight_decay=weight_decay, max_grad_norm=max_grad_norm, use_ema=True, ema_decay=EMA_DECAY,
                    overlap_update=overlap, master_weights=True)
    assert opt.overlap_update == overlap and len(bounds) == 2
    _run_steps(ops, model, opt, weight_decay, max_grad_norm, f"small wd={weight_decay} clip={max_grad_norm} overlap={overlap}", twin=True)
    assert (model.param_events is not None) == overlap


# ------------------------------------------------------------------------------------------------ b. range update
def test_master_step_range_update_leaves_the_rest_alone(ops):
    """An adapter set with module dropout updates ranges, each at its own step count (``update_ranges``): everything outside
    [8, n - 8) keeps planted bit patterns in all five buffers."""
    from yat_amd.optim import FlatAdamW
    starts, bounds, n = _layout(SMALL_SHAPES, SMALL_BUCKETS)
    model = _stand_in(starts, bounds, n, 0.5, seed=29)
    opt = FlatAdamW(model, lr=LR, weight_decay=0.01, max_grad_norm=1.0, use_ema=True, ema_decay=EMA_DECAY, master_weights=True)
    model.update_ranges = lambda: [(8, n - 8, opt.step_count)]
    outside = torch.ones(n, dtype=torch.bool, device=DEV)
    outside[8:n - 8] = False
    planted = {"flat_param": 0x7B5A}                           # bit patterns no update produces (large finite values)
    planted.update({k: 0x7B5A5A00 + i for i, k in enumerate(BUFFERS)})
    views = {"flat_param": model.flat_param.view(torch.int16)}
    views.update({k: getattr(opt, k).view(torch.int32) for k in BUFFERS})
    for k, v in views.items():
        v[outside] = planted[k]
    _run_steps(ops, model, opt, 0.01, 1.0, "range [8, n - 8)", sl=slice(8, n - 8))
    for k, v in views.items():
        assert (v[outside] == planted[k]).all(), f"{k}: an element outside the updated range was written"
    inside = slice(8, n - 8)
    assert torch.equal(model.flat_param[inside].view(torch.int16), opt.master[inside].to(BF).view(torch.int16))


# ------------------------------------------------------------------------------------------------ c. grid wrap
def test_master_step_past_one_grid_pass(ops):
    """One buffer of one grid pass + 8 x 1001 parameters: the capped grid wraps and its second pass ends ragged."""
    from yat_amd.optim import MASTER_GRID_PASS, FlatAdamW
    n = MASTER_GRID_PASS + 8 * 1001
    assert n > MASTER_GRID_PASS and (n // 8) % 2 == 1 and (n - MASTER_GRID_PASS) // 8 % 256 != 0
    model = _stand_in([0], [(0, n)], n, 0.02, seed=31)
    opt = FlatAdamW(model, lr=LR, weight_decay=0.01, max_grad_norm=1.0, use_ema=True, ema_decay=EMA_DECAY, master_weights=True)
    _run_steps(ops, model, opt, 0.01, 1.0, f"grid wrap n={n}")


# ------------------------------------------------------------------------------------------------ d. non-finite gradients
@pytest.mark.parametrize("bad", ["nan", "+inf", "-inf"])
def test_master_step_nonfinite_gradient_follows_torch(ops, bad):
    """One non-finite gradient element at step 2 of 3.  A NaN turns the coefficient and hence every value NaN; +-inf makes
    the coefficient 0, so that element's gradient is inf * 0 = NaN and the rest sees zero gradients.  torch's float32 run
    decides which positions of master, both moments, the shadow and the bf16 copy are NaN."""
    from yat_amd.optim import FlatAdamW
    starts, bounds, n = _layout(SMALL_SHAPES, SMALL_BUCKETS)
    model = _stand_in(starts, bounds, n, 0.5, seed=37)
    opt = FlatAdamW(model, lr=2e-2, weight_decay=0.01, max_grad_norm=1.0, use_ema=True, ema_decay=EMA_DECAY, master_weights=True)
    r32 = _Ref(model.flat_param, torch.float32, 2e-2, 0.01, warmup=0)
    value = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[bad]
    where = starts[3] + 17
    for step in range(1, 4):
        _fill_grad(model, 200 + step, 1.0 if step == 1 else 1e-3)
        if step == 2:
            model.flat_grad[where] = value
        g_cpu = model.flat_grad.cpu()
        opt.step()
        torch.cuda.synchronize()
        coef = _check_coef(opt, 1.0)
        print(f"[master] {bad} step {step}: norm {opt.grad_norm.item()!r} coef {coef!r}")
        if step == 2:
            assert math.isnan(coef) if bad == "nan" else coef == 0.0
        r32.step(g_cpu, coef)
        hip, ref = _hip_buffers(opt), r32.buffers()
        for k in BUFFERS:
            assert torch.equal(torch.isnan(hip[k]), torch.isnan(ref[k])), f"{bad} step {step} {k}: NaN positions differ from torch float32"
        assert torch.equal(torch.isnan(model.flat_param).cpu(), torch.isnan(ref["master"])), f"{bad} step {step}: bf16 copy"
        _assert_working_copy(model, opt, f"{bad} step {step}")
        finite = ~torch.isnan(ref["master"])
        if finite.any():                                       # the finite rest stays at torch's values (loose: the bars are above)
            assert torch.allclose(hip["master"][finite], ref["master"][finite], rtol=1e-5, atol=1e-7)
        r32.take(hip)
    nan_params = torch.isnan(opt.master).sum().item()
    assert nan_params == (n if bad == "nan" else 1)
