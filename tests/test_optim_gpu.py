"""Gradient-norm clip + AdamW (+ EMA) against torch where the kernels could go wrong unnoticed (GPU).

The product path is ``FlatAdamW.step``: ``yat_gradnorm_pieces_partial`` / ``_finish`` (the norm over pieces -- tensors cut at
the eighths of their bucket -- in 2^18-element chunks) and ``yat_adamw_step`` (csrc/optim.hip).  References are plain torch:
``get_total_norm`` / ``clip_grads_with_norm_`` (the two halves of ``clip_grad_norm_``), ``torch.optim.AdamW`` on bf16 CPU
tensors, ``oracle.recipe_ref.EMAModelRef``, and float64 sums where the kernel's own fp32 sums are checked.

* edge layouts: every partial slot against the float64 sum of squares of exactly its element range (fp32 summation of at
  most 2^18 squares: relative error <= 1e-5); norm and coefficient equal to a float64 restatement of the kernel's rounding
  points and within one bf16 ulp of torch;
* the real SANA-1.6B layout (396 tensors, 115-chunk tensors, tensors past one AdamW grid pass) and its split over 2, 4 and 8
  emulated ranks (bit for bit the one-rank norm);
* several AdamW + EMA steps at full width (every block bucket past one AdamW grid pass), bit-exact against torch CPU but for
  rare 1-ulp ties (<= 0.2 % of the elements, the bar of tests/test_kernels_gpu.py);
* non-finite gradients: NaN and +-inf give torch's norm, coefficient and NaN pattern.
"""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernels_gpu import BF, DEV, _collect_failures, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CHUNK = 1 << 18                     # csrc/optim.hip NORM_CHUNK
GRID_PASS = 8192 * 256 * 8          # elements one pass of the AdamW grid covers (csrc/optim.hip STEP_MAX_BLOCKS x 256 lanes x 8)

# ------------------------------------------------------------------------------------------------ helpers
def _up(x, a):
    return -(-x // a) * a


def _rb(x):
    """Round a float64 value through bf16 (the kernel's rbf)."""
    return torch.tensor(x, dtype=torch.float64).float().to(BF).double().item()


def _restate(tensor_sumsq, max_norm):
    """The finish kernels' rounding points on float64 per-tensor sums of squares: per-tensor norm -> bf16, sum of their
    squares -> sqrt -> bf16, max_norm / bf16(total + 1e-6) -> bf16, clamp at 1."""
    total = _rb(math.sqrt(sum(_rb(math.sqrt(s)) ** 2 for s in tensor_sumsq)))
    coef = _rb(max_norm / _rb(total + 1e-6))
    return total, min(coef, 1.0)


def _torch_coef(total, max_norm):
    """torch's clip coefficient for ``total`` (a bf16 tensor), read back through clip_grads_with_norm_ on a probe of ones."""
    probe = torch.nn.Parameter(torch.zeros(1, dtype=BF))
    probe.grad = torch.ones(1, dtype=BF)
    torch.nn.utils.clip_grads_with_norm_([probe], max_norm, total)
    return probe.grad.float().item()


def _torch_norm_coef(grads, max_norm):
    total = torch.nn.utils.get_total_norm(grads, 2.0)
    return total.float().item(), _torch_coef(total, max_norm)


def _within_ulp(a, b):
    """|a - b| <= one bf16 ulp at b (b finite, non-zero)."""
    return abs(a - b) <= 2.0 ** (math.floor(math.log2(abs(b))) - 7)


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _slot_ranges(piece_start, chunk_base):
    """(first, end) element of every partial slot, in slot order: chunk c of piece p is slot chunk_base[p] + c."""
    out = []
    for p in range(len(piece_start) - 1):
        a, b = piece_start[p], piece_start[p + 1]
        assert chunk_base[p + 1] - chunk_base[p] == -(-(b - a) // CHUNK)
        out += [(a + c * CHUNK, min(a + (c + 1) * CHUNK, b)) for c in range(chunk_base[p + 1] - chunk_base[p])]
    return out


def _check_tiling(ranges, n):
    assert ranges[0][0] == 0 and ranges[-1][1] == n
    assert all(r[1] == s[0] for r, s in zip(ranges[:-1], ranges[1:])), "slots do not tile the buffer"
    assert all(0 < b - a <= CHUNK for a, b in ranges)


def _f64_slots(g, ranges):
    """float64 sum of squares of every range (torch's reduction, on the device)."""
    return torch.stack([g[a:b].double().square().sum() for a, b in ranges])


def _slot_error(partial, ref, name, tol=1e-5):
    """Largest relative error of the kernel's fp32 slots against float64; a slot the kernel did not write stays NaN."""
    got = partial.double()
    assert torch.isfinite(got).all(), f"{name}: {(~torch.isfinite(got)).sum().item()} partial slots unwritten / non-finite"
    err = ((got - ref).abs() / ref.clamp_min(1e-300)).max().item()
    print(f"[optim] {name}: {ref.numel()} partial slots, largest relative error vs float64 {err:.3e}")
    assert err <= tol, f"{name}: partial slot error {err:.3e} > {tol}"
    return err


def _tensor_sums(ref, tensor_first, chunk_base):
    r = ref.tolist()
    return [sum(r[chunk_base[tensor_first[t]]:chunk_base[tensor_first[t + 1]]]) for t in range(len(tensor_first) - 1)]


def _compare(mine, ref, name, stats):
    """Same NaN positions; the other elements equal but for rare 1-ulp ties, counted into ``stats``.  A tie may differ by one
    bf16 ulp of the larger of the two values + 1e-3 of the tensor's mean magnitude (the relative part of
    test_kernels_gpu.close(): a tie upstream of a cancellation, p + update ~ 0, is one ulp of the operands, not of the result)."""
    mine, ref = mine.reshape(-1), ref.reshape(-1).to(mine.device)
    nm, nr = torch.isnan(mine), torch.isnan(ref)
    assert torch.equal(nm, nr), f"{name}: NaN at {nm.sum().item()} elements against torch's {nr.sum().item()}"
    a, b = mine[~nm].float(), ref[~nr].float()
    stats["n"] += mine.numel()
    if not a.numel():
        return
    stats["diff"] += (a != b).sum()
    m = torch.maximum(a.abs(), b.abs())
    ulp = torch.where(m > 0, torch.ldexp(torch.ones_like(m), torch.frexp(m).exponent - 8), torch.zeros_like(m))
    bound = ulp + 1e-3 * b.abs().mean()
    stats["excess"] = torch.maximum(stats["excess"], ((a - b).abs() - bound).max())


def _new_stats():
    return {"diff": torch.zeros((), dtype=torch.int64, device=DEV), "excess": torch.full((), -1.0, device=DEV), "n": 0}


def _assert_ties(stats, name):
    diff, excess = stats["diff"].item(), stats["excess"].item()
    print(f"[optim] {name}: {diff} / {stats['n']} elements differ from torch (1-ulp ties)")
    assert excess <= 0, f"{name}: an element beyond one bf16 ulp of torch by {excess:.3e}"
    assert diff <= 0.002 * stats["n"], f"{name}: {diff} of {stats['n']} elements differ from torch"
    return diff


def _fill_grads(model, seed, base):
    """Per-tensor scaled normal gradients (scales base * 4^-(i % 4)) drawn on the device."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    with torch.no_grad():
        for i, g in enumerate(model.G.values()):
            g.copy_(torch.randn(g.shape, generator=gen, device=DEV) * (base * 4.0 ** -(i % 4)))


# ------------------------------------------------------------------------------------------------ a. edge layouts
# buckets of tensor lengths: bucket starts at multiples of 64 elements (what flat.py's SHARD_ALIGN gives a model), tensors at
# multiples of 8; pad_end False leaves the last tensor unpadded, so its last chunk ends in a scalar tail and its bucket is not
# cut.  A length-0 tensor sits in every layout; 20 * 2^18 + 3 makes pieces of several chunks that start off chunk boundaries.
EDGE_LAYOUTS = {
    "eighths": ([[1, 7, 8], [CHUNK - 1, 0, CHUNK], [CHUNK + 1, 3 * CHUNK + 5], [20 * CHUNK + 3, 8]], True),
    "eighths_tail": ([[1, 7, 8, CHUNK - 1], [0, CHUNK, 20 * CHUNK + 3], [CHUNK + 1, 3 * CHUNK + 5]], False),
    "whole": ([[1, 7, 8, CHUNK - 1, 0, CHUNK, CHUNK + 1, 20 * CHUNK + 3, 3 * CHUNK + 5]], False),
}


def _edge_layout(buckets, pad_end):
    seg, lens, lows, off = [], [], [], 0
    for lens_b in buckets:
        off = _up(off, 64)
        lows.append(off)
        for L in lens_b:
            seg.append(off)
            lens.append(L)
            off += _up(L, 8)
    n = _up(off, 64) if pad_end else seg[-1] + lens[-1]
    return seg + [n], lens, list(zip(lows, lows[1:] + [n]))


@pytest.mark.parametrize("layout", list(EDGE_LAYOUTS))
def test_gradnorm_edge_layout(ops, layout):
    from yat_amd.optim import norm_pieces
    seg, lens, bounds = _edge_layout(*EDGE_LAYOUTS[layout])
    n, nt = seg[-1], len(lens)
    g = torch.zeros(n, dtype=BF, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(31)
    for i, (s, L) in enumerate(zip(seg, lens)):
        g[s:s + L] = (torch.randn(L, generator=gen, device=DEV) * 4.0 ** (i % 5 - 2)).to(BF)
    ps, tf, cb, mx, part = norm_pieces(seg, bounds)
    cut = [(lo, hi) for lo, hi in bounds if (hi - lo) % 64 == 0]
    assert bool(cut) == (layout != "whole") and mx > 1
    eighths = {lo + k * (hi - lo) // 8 for lo, hi in cut for k in range(8)}
    assert eighths <= set(ps), "an eighth of a bucket does not start a piece"
    ranges = _slot_ranges(ps, cb)
    _check_tiling(ranges, n)
    ref = _f64_slots(g, ranges)
    tsum = _tensor_sums(ref, tf, cb)
    grads_cpu = [g[s:s + L].cpu() for s, L in zip(seg, lens)]

    # pieces path (FlatAdamW)
    ps_d = torch.tensor(ps, dtype=torch.int64, device=DEV)
    tf_d, cb_d = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in (tf, cb))
    partial = torch.full((cb[-1],), float("nan"), device=DEV)
    ops.gradnorm_pieces_partial(g, ps_d, cb_d, mx, None, partial)
    _slot_error(partial, ref, f"{layout} pieces")

    # per-tensor entry point: workspace slot [t * maxchunks + c] holds chunk c of tensor t
    seg_d = torch.tensor(seg, dtype=torch.int64, device=DEV)
    mc = -(-n // CHUNK)
    ws = torch.full((ops.gradnorm_workspace_bytes(n, nt) // 4,), float("nan"), device=DEV)
    ranges_t = [(t, c, seg[t] + c * CHUNK, min(seg[t] + (c + 1) * CHUNK, seg[t + 1]))
                for t in range(nt) for c in range(-(-(seg[t + 1] - seg[t]) // CHUNK))]
    norm0, coef0 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.gradnorm_clip(g, seg_d, 1.0, norm0, coef0, ws)
    slots_t = ws[[t * mc + c for t, c, _, _ in ranges_t]]
    _slot_error(slots_t, _f64_slots(g, [(a, b) for _, _, a, b in ranges_t]), f"{layout} per-tensor")
    if layout == "whole":           # pieces are the tensors: both entry points hold the same bits in every slot
        assert len(ps) - 1 == sum(1 for L in lens if L)
        assert torch.equal(slots_t.view(torch.int32), partial.view(torch.int32))

    for max_norm in (1.0, 1e5):     # clipped, and clamped at 1
        norm1, coef1 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        ops.gradnorm_pieces_finish(tf_d, cb_d, partial, max_norm, norm1, coef1)
        ops.gradnorm_clip(g, seg_d, max_norm, norm0, coef0, ws)
        hn, hc, on, oc = norm1.item(), coef1.item(), norm0.item(), coef0.item()
        rn, rc = _restate(tsum, max_norm)
        tn, tc = _torch_norm_coef(grads_cpu, max_norm)
        print(f"[optim] {layout} max_norm={max_norm:g}: norm pieces={hn!r} per-tensor={on!r} float64={rn!r} torch={tn!r}; "
              f"coef pieces={hc!r} per-tensor={oc!r} float64={rc!r} torch={tc!r}")
        assert (hn, hc) == (rn, rc) and (on, oc) == (rn, rc)
        assert _within_ulp(hn, tn) and _within_ulp(hc, tc)
        assert (hc < 1.0) == (max_norm == 1.0)
        if layout == "whole":
            assert torch.equal(norm0.view(torch.int32), norm1.view(torch.int32))
            assert torch.equal(coef0.view(torch.int32), coef1.view(torch.int32))


# ------------------------------------------------------------------------------------------------ b. SANA-1.6B layout
@pytest.fixture(scope="module")
def sana_full():
    """SANA-1.6B's flat layout with random per-tensor-scaled gradients drawn on the device (the weights are not read)."""
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    hip = SanaTransformer2DModelHIP(SanaConfig(), device=DEV)
    _fill_grads(hip, seed=5, base=1e-3)
    yield hip
    del hip
    torch.cuda.empty_cache()


def test_gradnorm_sana_full_layout(ops, sana_full):
    from yat_amd.optim import FlatAdamW
    hip = sana_full
    numel = [g.numel() for g in hip.G.values()]
    # the layout exercises what the tiny models do not: more tensors than the finish kernel's 256 threads, tensors of many
    # chunks, tensors past one AdamW grid pass
    assert len(numel) == 396 and max(numel) > 100 * CHUNK and sum(x > GRID_PASS for x in numel) > 0
    opt = FlatAdamW(hip, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    opt.step()
    torch.cuda.synchronize()
    ps, tf, cb = opt._piece_start.tolist(), opt._tensor_first.tolist(), opt._chunk_base.tolist()
    ranges = _slot_ranges(ps, cb)
    _check_tiling(ranges, hip.numel_flat)
    ref = _f64_slots(hip.flat_grad, ranges)
    _slot_error(opt._partial, ref, "SANA-1.6B pieces")
    rn, rc = _restate(_tensor_sums(ref, tf, cb), 1.0)
    tn, tc = _torch_norm_coef([g.cpu() for g in hip.G.values()], 1.0)
    hn, hc = opt.grad_norm.item(), opt.clip_coef.item()
    print(f"[optim] SANA-1.6B: {len(numel)} tensors, {len(ps) - 1} pieces, {cb[-1]} slots; norm hip={hn!r} torch={tn!r} "
          f"float64={rn!r}; coef hip={hc!r} torch={tc!r} float64={rc!r}")
    assert (hn, hc) == (rn, rc)
    assert _within_ulp(hn, tn) and _within_ulp(hc, tc)
    assert hc < 1.0


@pytest.mark.parametrize("world", [2, 4, 8])
def test_gradnorm_sana_full_layout_split_over_ranks(ops, sana_full, world):
    """The sharded step: rank r sums the pieces it owns (``FlatAdamW._owned_mask``), the N partial arrays are added (the
    all-reduce), and the finish kernel gives the one-rank norm and coefficient bit for bit."""
    from yat_amd.optim import FlatAdamW
    hip = sana_full
    opt = FlatAdamW(hip, lr=1e-4, max_grad_norm=1.0)
    whole = torch.full_like(opt._partial, float("nan"))
    ops.gradnorm_pieces_partial(hip.flat_grad, opt._piece_start, opt._chunk_base, opt._max_chunks, None, whole)
    norm1, coef1 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.gradnorm_pieces_finish(opt._tensor_first, opt._chunk_base, whole, 1.0, norm1, coef1)
    nchunks = (opt._chunk_base[1:] - opt._chunk_base[:-1]).long()
    owners = torch.zeros_like(whole, dtype=torch.int32)
    total = torch.zeros_like(whole)
    for r in range(world):
        mask = opt._owned_mask(SimpleNamespace(rank=r, world=world, ddp=None)).clone()
        part = torch.full_like(whole, float("nan"))
        ops.gradnorm_pieces_partial(hip.flat_grad, opt._piece_start, opt._chunk_base, opt._max_chunks, mask, part)
        own = torch.repeat_interleave(mask.bool(), nchunks)
        owners += own.int()
        assert torch.equal(part[own].view(torch.int32), whole[own].view(torch.int32)), f"rank {r}: an owned slot differs"
        assert (part[~own] == 0).all(), f"rank {r}: a slot it does not own is not zero"
        total += part
    assert (owners == 1).all(), "a slot without exactly one owner"
    assert torch.equal(total.view(torch.int32), whole.view(torch.int32))
    norm, coef = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.gradnorm_pieces_finish(opt._tensor_first, opt._chunk_base, total, 1.0, norm, coef)
    print(f"[optim] world {world}: norm {norm.item()!r} coef {coef.item()!r} (one rank: {norm1.item()!r} {coef1.item()!r})")
    assert torch.equal(norm.view(torch.int32), norm1.view(torch.int32))
    assert torch.equal(coef.view(torch.int32), coef1.view(torch.int32))


# ------------------------------------------------------------------------------------------------ c. AdamW + EMA, full width
@pytest.fixture(scope="module")
def sana_wide():
    """SANA at full width, two blocks: 202 M parameters, every block bucket larger than one AdamW grid pass."""
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP
    hip = SanaTransformer2DModelHIP(SanaConfig(num_layers=2), device=DEV)
    yield hip
    del hip
    torch.cuda.empty_cache()


STEP_CASES = {
    "overlap": dict(overlap_update=True),                       # one launch per bucket on the optimizer stream
    "serial": dict(overlap_update=False),                       # one launch over the whole buffer
    "no_weight_decay": dict(weight_decay=0.0),
    "no_clip": dict(max_grad_norm=None, overlap_update=True),   # no coefficient passed
}
GRAD_BASE = (1e-3, 1e-6, 1e-3, 3e-4)     # per step: clipped, not clipped, clipped, ...
WARMUP, LR = 2, 1e-4                      # WarmupLR: the first step runs at lr = 0, the second at lr / 2


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_adamw_ema_steps_past_one_grid_pass(ops, sana_wide, case):
    """FlatAdamW(use_ema=True) + the trainer's WarmupLR against torch CPU AdamW + LambdaLR + EMAModelRef.  The clip
    coefficient is kept out of the AdamW comparison: the CPU side clips with HIP's norm (clip_grads_with_norm_), and the
    coefficient that gives is asserted equal to HIP's; the norm itself is held to torch by the tests above.  After each
    comparison torch's state takes HIP's values, so a 1-ulp tie is judged in the step that makes it and does not compound."""
    from oracle.recipe_ref import EMAModelRef
    from yat_amd.common.trainer import WarmupLR
    from yat_amd.optim import FlatAdamW
    kw = dict(weight_decay=0.01, max_grad_norm=1.0, overlap_update=False)
    kw.update(STEP_CASES[case])
    hip = sana_wide
    assert all(hi - lo > GRID_PASS for lo, hi in hip.bucket_bounds[1:])
    hip.init_synthetic(17)
    names = list(hip.P)
    params = [torch.nn.Parameter(hip.P[k].cpu().clone()) for k in names]
    ref = torch.optim.AdamW(params, lr=LR, weight_decay=kw["weight_decay"])
    ref_lr = torch.optim.lr_scheduler.LambdaLR(ref, lambda s: s / WARMUP if s < WARMUP else 1.0)
    ema = EMAModelRef(params, decay=0.999)
    opt = FlatAdamW(hip, lr=LR, use_ema=True, ema_decay=0.999, **kw)
    sched = WarmupLR(opt, WARMUP)
    stats = _new_stats()
    coefs = []
    for step, base in enumerate(GRAD_BASE, 1):
        _fill_grads(hip, seed=100 + step, base=base)
        for p, k in zip(params, names):
            p.grad = hip.G[k].cpu()
        lr = opt.param_groups[0]["lr"]
        assert abs(lr - ref_lr.get_last_lr()[0]) <= 1e-15 and (step > 1 or lr == 0.0)
        opt.step()
        sched.step()
        hip.join_pending_update()
        torch.cuda.synchronize()
        if kw["max_grad_norm"] is not None:
            total = torch.tensor(opt.grad_norm.item(), dtype=BF)
            assert total.float().item() == opt.grad_norm.item()
            coefs.append(opt.clip_coef.item())
            assert _torch_coef(total, kw["max_grad_norm"]) == coefs[-1]
            torch.nn.utils.clip_grads_with_norm_(params, kw["max_grad_norm"], total)
        ref.step()
        ref_lr.step()
        ema.step(params)
        assert opt._ema_decay_now() == ema.cur_decay_value
        for i, (p, k) in enumerate(zip(params, names)):
            o, n = hip._offset[k], p.numel()
            st = ref.state[p]
            pairs = ((hip.P[k], p.data, "parameter"), (opt.exp_avg[o:o + n], st["exp_avg"], "exp_avg"),
                     (opt.exp_avg_sq[o:o + n], st["exp_avg_sq"], "exp_avg_sq"),
                     (opt.ema_shadow[o:o + n], ema.shadow_params[i], "EMA shadow"))
            for mine, theirs, what in pairs:
                _compare(mine, theirs, f"step {step} {k} {what}", stats)
                theirs.copy_(mine.view(theirs.shape).cpu())   # both sides go on from the same state: a tie stays one step's
        print(f"[optim] {case} step {step}: lr={lr:g} coef={coefs[-1] if coefs else None} ema decay={ema.cur_decay_value:.6f}")
    if coefs:
        assert min(coefs) < 1.0 and max(coefs) == 1.0
    _assert_ties(stats, f"{case}: {len(GRAD_BASE)} steps x (parameters, exp_avg, exp_avg_sq, EMA shadow)")


# ------------------------------------------------------------------------------------------------ d. non-finite gradients
@pytest.mark.parametrize("bad", ["nan", "+inf", "-inf"])
def test_nonfinite_gradient_follows_torch(ops, bad):
    """One non-finite gradient element at step 2 of 3.  torch: a NaN makes the norm and the clip coefficient NaN
    (clamp(max=1) keeps a NaN), so every parameter, both moments and the EMA shadow turn NaN; +-inf gives coefficient 0, so
    only the element itself turns NaN (inf * 0) and the rest sees zero gradients.  Both entry points of the norm follow."""
    from oracle.recipe_ref import EMAModelRef
    from yat_amd.optim import FlatAdamW
    shapes = [(96, 40), (40,), (3, 3, 16), (2000,), (8,)]
    buckets = [[0, 1], [2, 3, 4]]
    starts, lows, off = [], [], 0
    for b in buckets:
        off = _up(off, 64)
        lows.append(off)
        for t in b:
            starts.append(off)
            off += _up(math.prod(shapes[t]), 8)
    off = _up(off, 64)
    g = torch.Generator().manual_seed(23)
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.5).to(BF)) for s in shapes]
    ref = torch.optim.AdamW(params, lr=2e-2, weight_decay=0.01)
    ema = EMAModelRef(params, decay=0.999)
    model = SimpleNamespace(flat_param=torch.zeros(off, dtype=BF, device=DEV), flat_grad=torch.zeros(off, dtype=BF, device=DEV),
                            seg_start=torch.tensor(starts + [off], dtype=torch.int64), numel_flat=off,
                            bucket_bounds=list(zip(lows, lows[1:] + [off])), param_events=None, join_pending_update=lambda: None)
    for p, s in zip(params, starts):
        model.flat_param[s:s + p.numel()] = p.data.flatten().to(DEV)
    hip = FlatAdamW(model, lr=2e-2, weight_decay=0.01, max_grad_norm=1.0, use_ema=True, ema_decay=0.999)
    assert all(part >= 0 for _, part in hip._piece_part)          # both buckets are cut into eighths
    ws = torch.empty(ops.gradnorm_workspace_bytes(off, len(shapes)), dtype=torch.uint8, device=DEV)
    norm0, coef0 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    value = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[bad]
    stats = _new_stats()
    for step in range(1, 4):
        for p, s in zip(params, starts):
            p.grad = (torch.randn(p.shape, generator=g) * (3.0 if step == 1 else 0.05)).to(BF)
            if step == 2 and p.numel() == 2000:
                p.grad[17] = value
            model.flat_grad[s:s + p.numel()] = p.grad.flatten().to(DEV)
        ops.gradnorm_clip(model.flat_grad, hip.seg_start, 1.0, norm0, coef0, ws)
        total = torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
        tn, tc = total.float().item(), _torch_coef(total, 1.0)
        ref.step()
        ema.step(params)
        hip.step()
        torch.cuda.synchronize()
        hn, hc, on, oc = hip.grad_norm.item(), hip.clip_coef.item(), norm0.item(), coef0.item()
        print(f"[optim] {bad} step {step}: norm hip={hn!r} per-tensor={on!r} torch={tn!r}; "
              f"coef hip={hc!r} per-tensor={oc!r} torch={tc!r}")
        assert _same(hn, tn) and _same(hc, tc), f"step {step}: norm / coefficient {hn!r} / {hc!r} against torch's {tn!r} / {tc!r}"
        assert _same(on, tn) and _same(oc, tc), f"step {step}: per-tensor entry point {on!r} / {oc!r} against {tn!r} / {tc!r}"
        for i, (p, s) in enumerate(zip(params, starts)):
            n, st = p.numel(), ref.state[p]
            _compare(model.flat_param[s:s + n], p.data, f"step {step} parameter {i}", stats)
            _compare(hip.exp_avg[s:s + n], st["exp_avg"], f"step {step} exp_avg {i}", stats)
            _compare(hip.exp_avg_sq[s:s + n], st["exp_avg_sq"], f"step {step} exp_avg_sq {i}", stats)
            _compare(hip.ema_shadow[s:s + n], ema.shadow_params[i], f"step {step} EMA shadow {i}", stats)
    nan_params = sum(torch.isnan(p.data).sum().item() for p in params)
    assert nan_params == (sum(p.numel() for p in params) if bad == "nan" else 1)      # torch's semantics, as stated above
    _assert_ties(stats, f"{bad}: 3 steps")
