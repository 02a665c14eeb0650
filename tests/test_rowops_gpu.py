"""The row and strip kernels (csrc/rowops.hip: LN+modulate, RMSNorm, gate backward, column sum, modulation table;
csrc/elementwise.hip: yat_transpose_bf16) at every dispatch class and ragged edge -- GPU.

Every reference is computed in fp64 on the CPU from the kernel's bf16 inputs, with rb() (round to bf16) applied at
exactly the points where the kernel, and the reference model's bf16 op flow, round.  Four kinds of check, none of
them measured on the code under test:

* close(hip, ref), defaults (rel L2 <= 2e-3, 2 bf16 ulps): outputs computed with the kernel's own rounding points
  (y, dlin, modulation_fwd).  rstd: close(tol=1e-5, ulps=0.01, atol=1e-7), one fp32 rsqrt of an fp32 mean.
  One rounding point is not decided by the inputs: the normalized row, rb(x * rstd) and rb((x - mean) * rstd), is rounded
  from an fp32 product whose two roundings (2 u |t|, u = 2^-24) can put it on the other side of a bf16 rounding boundary
  than the fp64 value -- one bf16 ulp of the normalized value, which `+ shift` can cancel down to many ulps of y.  The
  reference therefore takes the kernel's own fp32 mean / rstd (each held to fp64 separately), and where the fp64 value
  t lies within t (1 +- 2^-22) of a boundary it accepts either rounding (rb_either / nearer); everywhere else, and at
  every later rounding point (products and sums of bf16 values are exact in fp32), there is one reference value.
* as_good_as(hip, torch bf16 autograd, fp64 truth), defaults: the backward dx / dw / dshift / dscale of RMSNorm and
  LN (tol_flow=1e-2 for the column gradients dw, dshift, dscale).  The torch bf16 flow runs on the CPU as well.
* within(hip, ref64, bound): fp32 column accumulators whose terms the reference reproduces exactly (dgate: terms
  rb(dout * lin); modulation_bwd's dtmod: terms rb(g); the sum behind colsum, dbias and dtable: terms x, dlin, rb(g)).
  With u = 2^-24 (fp32 unit roundoff) and n the number of rows summed, any summation order obeys, per column,
      |sum_fp32 - sum_64| <= n * u * sum_r |term_r|.
  - fp32 output added onto a prior (`acc += sum`, one more fp32 addition):  + u * |prior + ref64|
  - bf16 output (one bf16 rounding of the fp32 sum):                        + 2^-8 * |ref64|
  - bf16 output with accumulate=1 (the kernel computes rb(sum) + prior, then rounds):
                                                                            + 2^-8 * |ref64| + 2^-8 * |prior + ref64|
* bit-exact: transpose, the slots of an accumulator table a call does not own, rows / elements past the logical
  extent (guard rows and tails hold a sentinel; input guards hold NaN, so a read past the extent poisons the result),
  mean / rstd of two launches, a call split in parts, and every output against what the workspace held before.

Workspaces are allocated with exactly the bytes the *_workspace_bytes entry declares and start as 0xFF bytes (NaN as
fp32): a partial row the first kernel does not write reaches the result.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_common import BF, DEV, _FAILS, _collect_failures, as_good_as, close, rb, rnd  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24                  # fp32 unit roundoff
ULP_BF = 2.0 ** -8                # one bf16 rounding, relative


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


# ------------------------------------------------------------------------------------------------ helpers
def d(t):
    return t.detach().cpu().double()


def _bits(t):
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


def same(a, b, name):
    """bit equality (NaN sentinels compare equal to themselves)"""
    if a.shape != b.shape or not torch.equal(_bits(a), _bits(b)):
        _FAILS.append(f"{name}: not bit-identical")
        print(f"[parity] {name}: NOT BIT-IDENTICAL")


def within(hip, ref, bound, name):
    hip = d(hip)
    if not torch.isfinite(hip).all():
        _FAILS.append(f"{name}: non-finite output")
        print(f"[parity] {name}: NON-FINITE")
        return
    err = (hip - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item() if bool((bound > 0).any()) else 0.0
    print(f"[parity] {name}: max_abs={err.max().item():.3e} worst err/bound={worst:.3f}")
    if bool((err > bound).any()):
        _FAILS.append(f"{name}: error exceeds the summation bound ({worst:.3f} x) at {int((err > bound).sum())} elements")


def rb_either(t):
    """the two bf16 values an fp32 evaluation of the fp64 value t may round to (equal except next to a rounding boundary)"""
    return rb(t * (1 - 2.0 ** -22)).double(), rb(t * (1 + 2.0 ** -22)).double()


def nearer(hip, a, b):
    hip = d(hip)
    print(f"[parity]   ({int((a != b).sum())} of {a.numel()} elements next to a rounding boundary of the normalized row)")
    return torch.where((hip - a).abs() <= (hip - b).abs(), a, b)


def guarded(t, fill, extra=3):
    """[M, ...] -> (whole [M + extra, ...] with `fill` in the guard rows, view of the first M rows)"""
    M = t.shape[0]
    whole = torch.full((M + extra, *t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    whole[:M] = t
    return whole, whole[:M]


def out_guarded(shape, dtype, fill=-1984.0, extra=3):
    whole = torch.full((shape[0] + extra, *shape[1:]), fill, dtype=dtype, device=DEV)
    return whole, whole[:shape[0]]


def guard_intact(whole, M, name, fill=-1984.0):
    same(whole[M:], torch.full_like(whole[M:], fill), f"{name} guard rows")


def wspace(nbytes):
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=DEV)


def bf16_sum_bound(n, terms_abs_sum, ref, prior=None):
    b = n * U32 * terms_abs_sum + ULP_BF * ref.abs()
    return b if prior is None else b + ULP_BF * (prior + ref).abs()


# ------------------------------------------------------------------------------------------------ 1. RMSNorm
@pytest.mark.parametrize("M", [1, 5, 16, 17, 67])
@pytest.mark.parametrize("D", [8, 72, 1024, 1032, 2560, 2568, 4096])
def test_rmsnorm_fwd_bwd(ops, D, M):
    """Both sides of every MAXV boundary (2 | 5 | 8 chunks of 512 columns per lane), the smallest D, a D with idle lanes;
    M below, at and off the 16 rows of a backward workgroup (the `row >= M` break and the all-zero partial rows)."""
    eps, tag = 1e-5, f"rmsnorm D={D} M={M}"
    nan = float("nan")
    xw, x = guarded(rnd(M, D, scale=1.5, seed=24), nan)
    dyw, dy = guarded(rnd(M, D, seed=25), nan)
    w = (1 + 0.1 * rnd(D, seed=26).float()).to(BF)
    yw, y = out_guarded((M, D), BF)
    rw, rstd = out_guarded((M,), torch.float32)
    ops.rmsnorm_fwd(x, w, eps, y=y, rstd=rstd)
    x64, w64 = d(x), d(w)
    r64 = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps)
    close(rstd.cpu(), r64[:, 0], f"{tag} rstd", tol=1e-5, ulps=0.01, atol=1e-7)
    y_ref = nearer(y, *(rb(xn * w64).double() for xn in rb_either(x64 * d(rstd)[:, None])))
    close(y.cpu(), y_ref, f"{tag} y")
    guard_intact(yw, M, f"{tag} y")
    guard_intact(rw, M, f"{tag} rstd")

    prior = rnd(D, scale=2.0, seed=27)

    def run(dt, dw0):      # diffusers RMSNorm op sequence (oracle/sana_ref.py RMSNorm); .grad accumulates like accumulate_dw
        xr, wr = (t.detach().cpu().to(dt).clone().requires_grad_(True) for t in (x, w))
        if dw0 is not None:
            wr.grad = dw0.cpu().to(dt).clone()
        var = xr.to(torch.float32 if dt is BF else dt).pow(2).mean(-1, keepdim=True)
        h = (xr * torch.rsqrt(var + eps)).to(dt) * wr
        h.backward(dy.cpu().to(dt))
        return xr.grad, wr.grad
    ws = wspace(ops._lib().yat_rmsnorm_bwd_workspace_bytes(M, D))
    dxs = []
    for acc in (False, True):
        flow, truth = run(BF, prior if acc else None), run(torch.float64, prior if acc else None)
        dxw, dx = out_guarded((M, D), BF)
        dw = prior.clone() if acc else torch.full((D,), nan, dtype=BF, device=DEV)
        ws.fill_(0xFF)
        ops.rmsnorm_bwd(x, w, rstd, dy, dx, dw, ws, accumulate_dw=acc)
        if not acc:
            as_good_as(dx.cpu(), flow[0], truth[0], f"{tag} dx")
        as_good_as(dw.cpu(), flow[1], truth[1], f"{tag} dw acc={int(acc)}", tol_flow=1e-2)
        guard_intact(dxw, M, f"{tag} dx acc={int(acc)}")
        dxs.append(dx)
    same(dxs[0], dxs[1], f"{tag} dx of the plain and the accumulating call")
    guard_intact(xw, M, f"{tag} x", fill=nan)
    guard_intact(dyw, M, f"{tag} dy", fill=nan)


# ------------------------------------------------------------------------------------------------ 2. gate backward
@pytest.mark.parametrize("B,rpb", [(1, 1), (3, 5), (2, 16), (2, 63), (1, 64), (2, 65), (3, 130)])
@pytest.mark.parametrize("D", [8, 264, 512, 520, 1152, 1536, 2240, 4096])
def test_gate_bwd(ops, D, B, rpb):
    """1 .. 8 column blocks of 512 (full and partly filled), rows per batch below / at / off the 16 rows of a wave and the
    64 of a workgroup, the gate in the last slot of a [B,6,D] and of a [B,9,D] table (gate_ld = acc_ld = 6 D | 9 D), a
    non-zero accumulator, and the fused bias gradient absent, plain and accumulating."""
    M, nan = B * rpb, float("nan")
    dout, lin = rnd(M, D, seed=29), rnd(M, D, seed=30)
    dout64 = d(dout)
    terms = rb(dout64 * d(lin)).double().view(B, rpb, D)                   # exact: a product of two bf16 fits fp32
    ws = wspace(ops._lib().yat_gate_bwd_workspace_bytes(M, D, rpb))
    for S in (6, 9):
        tag = f"gate_bwd D={D} B={B} rpb={rpb} S={S}"
        mod, prior = rnd(B, S, D, seed=31 + S), rnd(B, S, D, scale=3.0, seed=32 + S).float()
        gate = mod[:, S - 1]
        bias0 = rnd(D, scale=3.0, seed=33)
        res = []
        for mode in ("none", "plain", "acc"):
            dlin = torch.full((M, D), nan, dtype=BF, device=DEV)
            acc = prior.clone()
            dbias = None if mode == "none" else bias0.clone() if mode == "acc" else torch.full((D,), nan, dtype=BF, device=DEV)
            ws.fill_(0xFF)
            ops.gate_bwd(dout, lin, gate, S * D, rpb, dlin, acc[:, S - 1], S * D, ws, dbias=dbias,
                         accumulate_bias=mode == "acc")
            res.append((dlin, acc, dbias))
        (dlin, acc, _), (_, _, db_plain), (_, _, db_acc) = res
        for other, mode in zip(res[1:], ("plain", "accumulating")):
            same(other[0], dlin, f"{tag} dlin with {mode} dbias")
            same(other[1], acc, f"{tag} dgate with {mode} dbias")
        dlin_ref = rb(d(gate).repeat_interleave(rpb, 0) * dout64).double()  # exact, as above
        close(dlin.cpu(), dlin_ref, f"{tag} dlin")
        p64 = d(prior)
        ref = p64[:, S - 1] + terms.sum(1)
        within(acc[:, S - 1], ref, rpb * U32 * terms.abs().sum(1) + U32 * ref.abs(), f"{tag} dgate")
        same(acc[:, :S - 1], prior[:, :S - 1], f"{tag} slots the call does not own")
        bsum, babs = dlin_ref.sum(0), dlin_ref.abs().sum(0)
        within(db_plain, bsum, bf16_sum_bound(M, babs, bsum), f"{tag} dbias")
        within(db_acc, d(bias0) + bsum, bf16_sum_bound(M, babs, bsum, d(bias0)), f"{tag} dbias acc")


# ------------------------------------------------------------------------------------------------ 3. column sum
@pytest.mark.parametrize("rows", [1, 7, 127, 128, 129, 300])
@pytest.mark.parametrize("cols", [8, 504, 512, 520, 2240, 4608])
def test_colsum(ops, cols, rows):
    """Column blocks on either side of 512 and many of them; rows below one wave's 32, on either side of a workgroup's
    128 (one | two partial rows) and three row blocks (fewer partial rows than reduce threads); contiguous and as a
    column slice of a wider matrix whose neighbours hold large values; plain and accumulating."""
    x0 = rnd(rows, cols, seed=15)
    wide = torch.full((rows, cols + 64), 3.0e4, dtype=BF, device=DEV)
    wide[:, 32:32 + cols] = x0
    x64 = d(x0)
    ref, absum = x64.sum(0), x64.abs().sum(0)
    prior = rnd(cols, scale=3.0, seed=16)
    ws = wspace(ops._lib().yat_colsum_workspace_bytes(rows, cols))
    for name, x in (("contiguous", x0), ("slice", wide[:, 32:32 + cols])):
        for acc in (False, True):
            tag = f"colsum {rows}x{cols} {name} acc={int(acc)}"
            outw, out = out_guarded((cols,), BF, extra=8)
            out.copy_(prior) if acc else out.fill_(float("nan"))
            ws.fill_(0xFF)
            ops.colsum(x, out, ws, accumulate=acc)
            within(out, d(prior) + ref if acc else ref, bf16_sum_bound(rows, absum, ref, d(prior) if acc else None), tag)
            guard_intact(outw, cols, tag)


# ------------------------------------------------------------------------------------------------ 4. LN + modulate
def _ln_check(x, shift, scale, eps, n, y, mean, rstd, tag):
    x64 = d(x)
    m64 = x64.mean(-1)
    within(mean, m64, U32 * x64.abs().sum(-1) + 2 * U32 * m64.abs(), f"{tag} mean")      # D terms / D, one division
    close(rstd.cpu(), torch.rsqrt((x64 - m64[:, None]).pow(2).mean(-1) + eps), f"{tag} rstd", tol=1e-5, ulps=0.01, atol=1e-7)
    sc = rb(1 + d(scale)).double().repeat_interleave(n, 0)
    sh = d(shift).repeat_interleave(n, 0)
    t = (x64 - d(mean)[:, None]) * d(rstd)[:, None]
    y_ref = nearer(y, *(rb(rb(xh * sc).double() + sh).double() for xh in rb_either(t)))  # xh: F.layer_norm output (bf16)
    close(y.cpu(), y_ref, f"{tag} y")


@pytest.mark.parametrize("B,rpb", [(1, 1), (2, 15), (2, 63), (1, 64), (2, 65), (2, 130)])
@pytest.mark.parametrize("D", [8, 1024, 1032, 2560, 2568])
def test_ln_modulate_fwd_bwd(ops, D, B, rpb):
    """Rows per batch on either side of the 64 rows of a column-pass workgroup (gridDim.y = 1 | 2 | 3, the out-of-range
    rows of the last one), both sides of the MAXV boundaries, shift / scale in a [B,6,D] and in a [B,9,D] table, non-zero
    accumulators, with and without the residual gradient."""
    M, eps, nan = B * rpb, 1e-6, float("nan")
    x = rnd(M, D, scale=2.0, seed=20) + 0.5
    dy, dres = rnd(M, D, seed=22), rnd(M, D, seed=23)
    ws = wspace(ops.ln_bwd_workspace_bytes(M, D, rpb))
    for S in (6, 9):
        tag = f"ln D={D} B={B} rpb={rpb} S={S}"
        mod = rnd(B, S, D, scale=0.3, seed=21 + S)
        i_sh, i_sc = S - 3, S - 2
        shift, scale = mod[:, i_sh], mod[:, i_sc]
        yw, y = out_guarded((M, D), BF)
        _, mean, rstd = ops.ln_modulate_fwd(x, shift, scale, S * D, rpb, eps, y=y)
        _ln_check(x, shift, scale, eps, rpb, y, mean, rstd, tag)
        guard_intact(yw, M, f"{tag} y")
        y2, mean2, rstd2 = ops.ln_modulate_fwd(x, shift, scale, S * D, rpb, eps, y=torch.zeros_like(x))
        same(y2, y, f"{tag} y of a second launch")
        same(mean2, mean, f"{tag} mean of a second launch")
        same(rstd2, rstd, f"{tag} rstd of a second launch")

        def run(dt):       # the reference's op sequence: norm(x) * (1 + scale[:, None]) + shift[:, None]
            xr, scr, shr = (t.detach().cpu().to(dt).clone().requires_grad_(True) for t in (x, scale, shift))
            yr = F.layer_norm(xr, (D,), None, None, eps).view(B, rpb, D) * (1 + scr)[:, None] + shr[:, None]
            yr.backward(dy.cpu().to(dt).view(B, rpb, D))
            return xr.grad, xr.grad + dres.cpu().to(dt), shr.grad, scr.grad
        flow, truth = run(BF), run(torch.float64)
        prior = rnd(B, S, D, scale=3.0, seed=40 + S).float()
        dxw, dx = out_guarded((M, D), BF)
        acc = prior.clone()
        ws.fill_(0xFF)
        ops.ln_modulate_bwd(x, mean, rstd, scale, S * D, rpb, dy, dres, dx, acc[:, i_sh], acc[:, i_sc], S * D, ws)
        as_good_as(dx.cpu(), flow[1], truth[1], f"{tag} dx+dres")
        guard_intact(dxw, M, f"{tag} dx")
        p64 = d(prior)
        as_good_as(d(acc[:, i_sh]) - p64[:, i_sh], flow[2], truth[2], f"{tag} dshift", tol_flow=1e-2)
        as_good_as(d(acc[:, i_sc]) - p64[:, i_sc], flow[3], truth[3], f"{tag} dscale", tol_flow=1e-2)
        own = [i for i in range(S) if i not in (i_sh, i_sc)]
        same(acc[:, own], prior[:, own], f"{tag} slots the call does not own")
        dx0 = torch.full_like(x, nan)
        ops.ln_modulate_bwd(x, mean, rstd, scale, S * D, rpb, dy, None, dx0, acc[:, i_sh], acc[:, i_sc], S * D, ws, parts=1)
        as_good_as(dx0.cpu(), flow[0], truth[0], f"{tag} dx")
        # the two halves launched separately (dx on the dependent chain, shift/scale gradients elsewhere) give the same bits
        dx_p, acc_p = torch.full_like(x, nan), prior.clone()
        ws.fill_(0xFF)
        ops.ln_modulate_bwd(x, mean, rstd, scale, S * D, rpb, dy, dres, dx_p, acc_p[:, i_sh], acc_p[:, i_sc], S * D, ws, parts=1)
        same(dx_p, dx, f"{tag} dx of parts=1")
        same(acc_p, prior, f"{tag} accumulators after parts=1")
        ops.ln_modulate_bwd(x, mean, rstd, scale, S * D, rpb, dy, None, None, acc_p[:, i_sh], acc_p[:, i_sc], S * D, ws, parts=2)
        same(acc_p, acc, f"{tag} accumulators of parts=2")


# ------------------------------------------------------------------------------------------------ 5. modulation table
@pytest.mark.parametrize("B,S,D", [(1, 6, 8), (3, 6, 136), (2, 9, 1536), (5, 2, 264)])
def test_modulation_fwd_bwd(ops, B, S, D):
    """tmod / dtmod as views of a wider buffer (row stride > S D, padding untouched), slot_stride = D (one row per slot) and
    0 (every slot adds the same row), the table gradient plain and accumulating, a non-zero dtmod."""
    PAD, nan = 40, float("nan")
    table = rnd(S, D, seed=26)
    dmod = rnd(B, S, D, seed=29).float() + 1e-3 * rnd(B, S, D, seed=30).float()      # fp32 values that are no bf16
    g = rb(d(dmod)).double()                                                         # what each consumer is handed
    tab0 = rnd(S, D, scale=3.0, seed=31)
    for stride in (D, 0):
        W = S * D if stride else D
        tag = f"modulation B={B} S={S} D={D} slot_stride={stride}"
        tw = torch.full((B, W + PAD), 3.0e4, dtype=BF, device=DEV)
        tw[:, :W] = rnd(B, W, seed=27)
        tmod = tw[:, :W]
        outw, out = out_guarded((B, S, D), BF)
        ops.modulation_fwd(table, tmod, stride, out=out)
        t64 = d(tmod).view(B, S, D) if stride else d(tmod)[:, None]
        close(out.cpu(), rb(d(table)[None] + t64), f"{tag} fwd")
        guard_intact(outw, B, f"{tag} fwd")
        for acc in (False, True):
            dtw = rnd(B, W + PAD, scale=3.0, seed=32).float()
            dt_prior = dtw.clone()
            dtab = tab0.clone() if acc else torch.full((S, D), nan, dtype=BF, device=DEV)
            ops.modulation_bwd(dmod, dtab, dtw[:, :W], stride, accumulate_table=acc)
            tsum, tabs = g.sum(0), g.abs().sum(0)
            within(dtab, d(tab0) + tsum if acc else tsum, bf16_sum_bound(B, tabs, tsum, d(tab0) if acc else None),
                   f"{tag} dtable acc={int(acc)}")
            terms = g.view(B, 1, W) if stride else g                                 # [B, n, W]: n terms per dtmod element
            n = terms.shape[1]
            ref = d(dt_prior)[:, :W] + terms.sum(1)
            within(dtw[:, :W], ref, n * U32 * terms.abs().sum(1) + U32 * ref.abs(), f"{tag} dtmod acc={int(acc)}")
            same(dtw[:, W:], dt_prior[:, W:], f"{tag} dtmod padding")
        same(tw[:, W:], torch.full_like(tw[:, W:], 3.0e4), f"{tag} tmod padding")


# ------------------------------------------------------------------------------------------------ 6. transpose
@pytest.mark.parametrize("B,R,C", [(1, 1, 1), (2, 33, 31), (3, 64, 32), (2, 100, 4), (2, 7, 65), (1, 1024, 32)])
def test_transpose(ops, B, R, C):
    """One element, tiles ragged in either direction, whole tiles, a thin and a wide matrix, 32 row tiles."""
    TAIL, n = 64, B * R * C
    x = rnd(B, R, C, seed=70)
    flat = torch.full((n + TAIL,), -1984.0, dtype=BF, device=DEV)
    out = flat[:n].view(B, C, R)
    ops.transpose(x, out=out)
    same(out, x.transpose(1, 2).contiguous(), f"transpose {B}x{R}x{C}")
    same(flat[n:], torch.full((TAIL,), -1984.0, dtype=BF, device=DEV), f"transpose {B}x{R}x{C} tail")
    same(ops.transpose(out), x, f"transpose {B}x{R}x{C} twice")


# ------------------------------------------------------------------------------------------------ 7. workspace contract
GUARD = 4096


def _ws_contract(nbytes, run, name):
    """`run(workspace)` -> outputs.  Exactly the declared bytes, followed by a guard INSIDE the same allocation: the results
    do not depend on what the workspace held (zeros | 0xFF = NaN as fp32), are finite, and the guard keeps its bytes."""
    assert nbytes > 0, f"{name}: no workspace declared"
    results = []
    for fill in (0x00, 0xFF):
        buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=DEV)
        buf[:nbytes] = fill
        buf[nbytes:] = 0xA5
        outs = run(buf)
        same(buf[nbytes:], torch.full((GUARD,), 0xA5, dtype=torch.uint8, device=DEV), f"{name} guard after {nbytes} bytes")
        for i, o in enumerate(outs):
            if not torch.isfinite(o.float()).all():
                _FAILS.append(f"{name}: output {i} non-finite with workspace bytes {fill:#x}")
        results.append(outs)
    for i, (a, b) in enumerate(zip(*results)):
        same(a, b, f"{name} output {i} (workspace of zeros vs 0xFF)")
    print(f"[parity] {name}: {nbytes} workspace bytes, {len(results[0])} outputs compared")


@pytest.mark.parametrize("M,D", [(5, 72), (67, 2568), (4115, 72)])
def test_workspace_rmsnorm_bwd(ops, M, D):
    """(4115 rows: 258 groups of 16 rows on the 256 workgroups the backward is capped at -- one partial row per workgroup)"""
    x, dy, w = rnd(M, D, scale=1.5, seed=24), rnd(M, D, seed=25), (1 + 0.1 * rnd(D, seed=26).float()).to(BF)
    _, rstd = ops.rmsnorm_fwd(x, w, 1e-5)

    def run(ws):
        dx, dw = torch.zeros_like(x), torch.zeros_like(w)
        ops.rmsnorm_bwd(x, w, rstd, dy, dx, dw, ws)
        return dx, dw
    _ws_contract(int(ops._lib().yat_rmsnorm_bwd_workspace_bytes(M, D)), run, f"workspace rmsnorm_bwd {M}x{D}")


@pytest.mark.parametrize("B,rpb,D", [(2, 15, 1032), (2, 130, 2568)])
def test_workspace_ln_bwd(ops, B, rpb, D):
    M = B * rpb
    x, dy, mod = rnd(M, D, scale=2.0, seed=20) + 0.5, rnd(M, D, seed=22), rnd(B, 6, D, scale=0.3, seed=27)
    _, mean, rstd = ops.ln_modulate_fwd(x, mod[:, 3], mod[:, 4], 6 * D, rpb, 1e-6)
    prior = rnd(B, 6, D, seed=46).float()

    def run(ws):
        dx, acc = torch.zeros_like(x), prior.clone()
        ops.ln_modulate_bwd(x, mean, rstd, mod[:, 4], 6 * D, rpb, dy, None, dx, acc[:, 3], acc[:, 4], 6 * D, ws)
        return dx, acc
    _ws_contract(ops.ln_bwd_workspace_bytes(M, D, rpb), run, f"workspace ln_bwd B={B} rpb={rpb} D={D}")


@pytest.mark.parametrize("rows,cols", [(7, 520), (300, 2240)])
def test_workspace_colsum(ops, rows, cols):
    x = rnd(rows, cols, seed=15)

    def run(ws):
        out = torch.zeros(cols, dtype=BF, device=DEV)
        ops.colsum(x, out, ws)
        return (out,)
    _ws_contract(int(ops._lib().yat_colsum_workspace_bytes(rows, cols)), run, f"workspace colsum {rows}x{cols}")


@pytest.mark.parametrize("B,rpb,D", [(2, 16, 264), (3, 130, 1536)])
def test_workspace_gate_bwd(ops, B, rpb, D):
    M = B * rpb
    dout, lin, mod = rnd(M, D, seed=29), rnd(M, D, seed=30), rnd(B, 6, D, seed=37)
    prior = rnd(B, 6, D, seed=38).float()

    def run(ws):
        dlin, acc, dbias = torch.zeros_like(dout), prior.clone(), torch.zeros(D, dtype=BF, device=DEV)
        ops.gate_bwd(dout, lin, mod[:, 5], 6 * D, rpb, dlin, acc[:, 5], 6 * D, ws, dbias=dbias)
        return dlin, acc, dbias
    _ws_contract(int(ops._lib().yat_gate_bwd_workspace_bytes(M, D, rpb)), run, f"workspace gate_bwd B={B} rpb={rpb} D={D}")


# ------------------------------------------------------------------------------------------------ 8. argument rejection
def _rejected(call, outputs, name):
    """`call()` must raise before any launch: every pre-filled output keeps its bits."""
    from yat_amd import lib as L
    before = [o.clone() for o in outputs]
    with pytest.raises(L.YatLibraryError):
        call()
    torch.cuda.synchronize()
    for i, (o, b) in enumerate(zip(outputs, before)):
        same(o, b, f"{name} output {i} after the rejected call")


@pytest.mark.parametrize("D", [12, 4104])
def test_rejects_row_width(ops, D):
    """D off a multiple of 8 or beyond the 4096 columns a wave holds: RMSNorm and LN return before any launch."""
    M = 4
    x, dy, w = rnd(M, D, seed=1), rnd(M, D, seed=2), rnd(D, seed=3)
    stat = lambda: torch.full((M,), 0.5, device=DEV)                                    # noqa: E731
    ws = wspace(1 << 20)
    y, rstd = rnd(M, D, seed=5), stat()
    _rejected(lambda: ops.rmsnorm_fwd(x, w, 1e-5, y=y, rstd=rstd), [y, rstd], f"rmsnorm_fwd D={D}")
    dx, dw = rnd(M, D, seed=6), rnd(D, seed=7)
    _rejected(lambda: ops.rmsnorm_bwd(x, w, rstd, dy, dx, dw, ws), [dx, dw], f"rmsnorm_bwd D={D}")
    mod_ld = (6 * D + 7) // 8 * 8                                                       # (mod_ld itself passes its own check)
    modp = torch.zeros(mod_ld, dtype=BF, device=DEV)
    mean = stat()
    _rejected(lambda: ops.ln_modulate_fwd(x, modp, modp, mod_ld, M, 1e-6, y=y, mean=mean, rstd=rstd), [y, mean, rstd],
              f"ln_modulate_fwd D={D}")
    acc = rnd(1, mod_ld, seed=8).float()
    for parts in ((3, 2) if D & 7 else (3,)):       # (the column pass alone has no 4096 limit, but loads 8 columns at once)
        _rejected(lambda: ops.ln_modulate_bwd(x, mean, rstd, modp, mod_ld, M, dy, None, dx, acc[:, :D], acc[:, D:2 * D],
                                              mod_ld, ws, parts=parts), [dx, acc], f"ln_modulate_bwd D={D} parts={parts}")


def test_rejects_ragged_batches_and_columns(ops):
    """M off a multiple of rows_per_batch (gate backward, LN backward) and a column count off a multiple of 8 (column
    sum) return before any launch."""
    M, D, rpb = 10, 64, 4
    x, dy, mod = rnd(M, D, seed=1), rnd(M, D, seed=2), rnd(3, 6, D, seed=3)
    ws = wspace(1 << 20)
    dlin, acc = rnd(M, D, seed=4), rnd(3, 6, D, seed=5).float()
    dbias = rnd(D, seed=6)
    _rejected(lambda: ops.gate_bwd(x, dy, mod[:, 5], 6 * D, rpb, dlin, acc[:, 5], 6 * D, ws, dbias=dbias),
              [dlin, acc, dbias], "gate_bwd M % rpb")
    stat = torch.full((M,), 0.5, device=DEV)
    dx = rnd(M, D, seed=7)
    _rejected(lambda: ops.ln_modulate_bwd(x, stat, stat, mod[:, 4], 6 * D, rpb, dy, None, dx, acc[:, 3], acc[:, 4], 6 * D, ws),
              [dx, acc], "ln_modulate_bwd M % rpb")
    out = rnd(16, seed=8)
    _rejected(lambda: ops.colsum(rnd(8, 16, seed=9)[:, :12], out, ws), [out], "colsum cols=12")
