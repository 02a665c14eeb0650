"""The strided, segmented RMSNorm pair (csrc/rowops.hip: yat_rmsnorm_seg_fwd / yat_rmsnorm_seg_bwd, the q/k norm of
SANA-1.5) at every dispatch class, ragged edge, leading dimension and aliasing mode -- GPU.

Same references and bars as tests/test_rowops_gpu.py::test_rmsnorm_fwd_bwd holds yat_rmsnorm_fwd / _bwd to (its docstring
derives them): rstd against fp64 with close(tol=1e-5, ulps=0.01, atol=1e-7); y against the two-rounding fp64 restatement with
the kernel's own rstd and either rounding accepted next to a rounding boundary of the normalised row (rb_either / nearer);
dx and dw with as_good_as against torch's bf16 autograd flow and the fp64 truth (tol_flow=1e-2 for dw).  Every operand sits
in a buffer with NaN guard rows and NaN guard columns between nseg * D and the leading dimension; every output in one filled
with a sentinel, which must be intact afterwards; workspaces hold exactly the declared bytes and start as 0xFF.  The two
segments of a row get different scales (1.5 and 0.25) and different weights, so a segment normalised with the other one's
rstd or weight fails.
"""
import pytest
import torch

from tests.gpu_common import BF, DEV, _FAILS, _collect_failures, as_good_as, close, rb, rnd  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAN = float("nan")
SENT = -1984.0
SCALES = (1.5, 0.25)


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


def rb_either(t):
    """the two bf16 values an fp32 evaluation of the fp64 value t may round to (equal except next to a rounding boundary)"""
    return rb(t * (1 - 2.0 ** -22)).double(), rb(t * (1 + 2.0 ** -22)).double()


def nearer(hip, a, b):
    hip = d(hip)
    print(f"[parity]   ({int((a != b).sum())} of {a.numel()} elements next to a rounding boundary of the normalized row)")
    return torch.where((hip - a).abs() <= (hip - b).abs(), a, b)


def guarded(t, fill, ld=None, off=0, extra=3):
    """[M, W] -> (whole [M + extra, ld] full of `fill` with t at rows [0, M), columns [off, off + W); that view).  The guard
    rows and the guard columns between W and ld hold `fill`."""
    M, W = t.shape
    ld = W if ld is None else ld
    whole = torch.full((M + extra, ld), fill, dtype=t.dtype, device=DEV)
    whole[:M, off:off + W] = t
    return whole, whole[:M, off:off + W]


def out_guarded(shape, dtype, fill=SENT, extra=3):
    whole = torch.full((shape[0] + extra, *shape[1:]), fill, dtype=dtype, device=DEV)
    return whole, whole[:shape[0]]


def guard_intact(whole, view, name, fill):
    """every element of `whole` outside `view` (guard rows and guard columns) still holds `fill`, bit for bit"""
    M, W = view.shape
    off = view.storage_offset() - whole.storage_offset()
    probe = whole.clone()
    probe[:M, off:off + W] = fill
    same(probe, torch.full_like(whole, fill), f"{name} guard rows / columns")


def wspace(nbytes):
    return torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=DEV)


# (4115 rows: 258 groups of 16 rows for the 256 workgroups of the backward -- two of them walk a second group, one of these
#  a ragged one)
CASES = [(D, 17) for D in (8, 72, 1024, 1032, 2240, 2560, 2568, 4096)] + \
        [(D, M) for D in (72, 2568) for M in (1, 5, 16, 67)] + [(72, 4115)]


# ------------------------------------------------------------------------------------------------ forward + backward
@pytest.mark.parametrize("nseg", [1, 2])
@pytest.mark.parametrize("D,M", CASES)
def test_rmsnorm_seg_fwd_bwd(ops, D, M, nseg):
    """Both sides of every MAXV class (2 | 5 | 8 chunks of 512 columns per lane), the smallest D, a D with idle lanes and the
    model's 2240; M below, at and off the 4 tasks of a forward workgroup and the 16 rows of a backward one, and past the 4096
    rows at which the backward's workgroups start to stride over row groups.  Four layouts:
    compact, q|k of a [M, 3D] projection in place (with and without the raw copy), and a [M, 3D + 8] matrix with the segments
    at its right edge, out of place."""
    W = nseg * D
    xs = [rnd(M, D, scale=SCALES[s], seed=24 + 10 * s) for s in range(nseg)]
    dys = [rnd(M, D, seed=25 + 10 * s) for s in range(nseg)]
    ws_ = [((1.0, 0.6)[s] + 0.1 * rnd(D, seed=26 + 10 * s).float()).to(BF) for s in range(nseg)]
    priors = [rnd(D, scale=2.0, seed=27 + 10 * s) for s in range(nseg)]
    x_all, dy_all = torch.cat(xs, 1), torch.cat(dys, 1)
    x64 = [d(x) for x in xs]
    r64 = torch.stack([torch.rsqrt(x.pow(2).mean(-1) + EPS) for x in x64], 1)                      # [M, nseg]

    def run(s, dt, dw0):      # diffusers RMSNorm op sequence (oracle/sana_ref.py RMSNorm); .grad accumulates like accumulate_dw
        xr, wr = (t.detach().cpu().to(dt).clone().requires_grad_(True) for t in (xs[s], ws_[s]))
        if dw0 is not None:
            wr.grad = dw0.cpu().to(dt).clone()
        var = xr.to(torch.float32 if dt is BF else dt).pow(2).mean(-1, keepdim=True)
        h = (xr * torch.rsqrt(var + EPS)).to(dt) * wr
        h.backward(dys[s].cpu().to(dt))
        return xr.grad, wr.grad
    refs = {(s, acc): (run(s, BF, priors[s] if acc else None), run(s, torch.float64, priors[s] if acc else None))
            for s in range(nseg) for acc in (False, True)}

    ws = wspace(ops.rmsnorm_seg_bwd_workspace_bytes(M, D, nseg))
    #          ld,        column offset, in place, keep
    layouts = [(W,         0,             False,    True),
               (3 * D,     0,             True,     True),
               (3 * D,     0,             True,     False),
               (3 * D + 8, 3 * D + 8 - W, False,    False)]
    first = {}
    for ld, off, inplace, keep in layouts:
        tag = f"rmsnorm_seg D={D} M={M} nseg={nseg} ld={ld} {'in place' if inplace else 'out of place'} keep={int(keep)}"
        xw, x = guarded(x_all, NAN, ld, off)
        yw, y = (xw, x) if inplace else guarded(torch.full_like(x_all, SENT), SENT, ld, off)
        kw, kp = out_guarded((M, W), BF) if keep else (None, None)
        rw, rstd = out_guarded((M, nseg), torch.float32)
        ops.rmsnorm_seg_fwd(x, ws_, EPS, y, rstd, keep=kp)
        close(rstd.cpu(), r64, f"{tag} rstd", tol=1e-5, ulps=0.01, atol=1e-7)
        for s in range(nseg):
            ys = y[:, s * D:(s + 1) * D]
            y_ref = nearer(ys, *(rb(xn * d(ws_[s])).double() for xn in rb_either(x64[s] * d(rstd)[:, s:s + 1])))
            close(ys.cpu(), y_ref, f"{tag} y segment {s}")
        guard_intact(yw, y, f"{tag} y", NAN if inplace else SENT)
        guard_intact(rw, rstd, f"{tag} rstd", SENT)
        if keep:
            same(kp, x_all, f"{tag} kept raw input")
            guard_intact(kw, kp, f"{tag} keep", SENT)
        if not inplace:
            same(x, x_all, f"{tag} x after the call")
            guard_intact(xw, x, f"{tag} x", NAN)
        for k, v in (("y", y), ("rstd", rstd)):                 # the layout changes addresses, not arithmetic
            if k in first:
                same(v, first[k], f"{tag} {k} vs the compact layout")
            else:
                first[k] = v.clone()

        # backward: the raw input from the keep buffer (compact) or from a strided copy with NaN guards of its own
        rxw, rx = (kw, kp) if keep else guarded(x_all, NAN, ld, off)
        dxs = []
        for mode in ("plain", "accumulate", "no dw"):
            acc = mode == "accumulate"
            dyw, dy = guarded(dy_all, NAN, ld, off)
            dxw, dx = (dyw, dy) if inplace else guarded(torch.full_like(dy_all, SENT), SENT, ld, off)
            dws = None if mode == "no dw" else [priors[s].clone() if acc else torch.full((D,), NAN, dtype=BF, device=DEV)
                                               for s in range(nseg)]
            ws.fill_(0xFF)
            ops.rmsnorm_seg_bwd(rx, ws_, rstd, dy, dx, dws, None if dws is None else ws, accumulate_dw=acc)
            for s in range(nseg):
                flow, truth = refs[(s, acc)]
                if mode == "plain":
                    as_good_as(dx[:, s * D:(s + 1) * D].cpu(), flow[0], truth[0], f"{tag} dx segment {s}")
                if dws is not None:
                    as_good_as(dws[s].cpu(), flow[1], truth[1], f"{tag} dw segment {s} acc={int(acc)}", tol_flow=1e-2)
            guard_intact(dxw, dx, f"{tag} dx ({mode})", NAN if inplace else SENT)
            if not inplace:
                same(dy, dy_all, f"{tag} dy after the call ({mode})")
                guard_intact(dyw, dy, f"{tag} dy ({mode})", NAN)
            dxs.append(dx.clone())
            if mode != "no dw":
                key = f"dw acc={int(acc)}"
                if key in first:
                    for s in range(nseg):
                        same(dws[s], first[key][s], f"{tag} {key} segment {s} vs the compact layout")
                else:
                    first[key] = [t.clone() for t in dws]
        same(dxs[0], dxs[1], f"{tag} dx of the plain and the accumulating call")
        same(dxs[0], dxs[2], f"{tag} dx of the plain call and the call without dw")
        if "dx" in first:
            same(dxs[0], first["dx"], f"{tag} dx vs the compact layout")
        else:
            first["dx"] = dxs[0]
        same(rx, x_all, f"{tag} raw input after the backward")
        guard_intact(rxw, rx, f"{tag} raw input", SENT if keep else NAN)


@pytest.mark.parametrize("accumulate_dw", [False, True])
@pytest.mark.parametrize("D,M", [(72, 37), (2240, 37), (4096, 37), (72, 4115)])
def test_one_segment_is_the_plain_rmsnorm(ops, D, M, accumulate_dw):
    """yat_rmsnorm_fwd / _bwd are the segment kernels at nseg = 1 on compact rows: y, rstd, dx and dw bit for bit, dw written
    plainly and accumulated onto a non-zero prior, out of a workspace of the same declared size.  One MAXV class each at 37
    rows, and 4115 rows of 72 columns: 258 row groups on the 256 workgroups of the backward, so two workgroups walk a second
    group and one of these a ragged one."""
    x, dy, w = rnd(M, D, scale=1.5, seed=24), rnd(M, D, seed=25), (1 + 0.1 * rnd(D, seed=26).float()).to(BF)
    y0, r0 = ops.rmsnorm_fwd(x, w, EPS)
    y1, r1 = torch.empty_like(x), torch.empty(M, dtype=torch.float32, device=DEV)
    ops.rmsnorm_seg_fwd(x, [w], EPS, y1, r1)
    same(y1, y0, "y")
    same(r1, r0, "rstd")
    nbytes = ops._lib().yat_rmsnorm_bwd_workspace_bytes(M, D)
    assert nbytes == ops.rmsnorm_seg_bwd_workspace_bytes(M, D, 1)
    prior = rnd(D, scale=2.0, seed=27)
    dx0, dx1 = torch.empty_like(x), torch.empty_like(x)
    dw0, dw1 = (prior.clone() if accumulate_dw else torch.full((D,), NAN, dtype=BF, device=DEV) for _ in range(2))
    ops.rmsnorm_bwd(x, w, r0, dy, dx0, dw0, wspace(nbytes), accumulate_dw=accumulate_dw)
    ops.rmsnorm_seg_bwd(x, [w], r1, dy, dx1, [dw1], wspace(nbytes), accumulate_dw=accumulate_dw)
    same(dx1, dx0, "dx")
    same(dw1, dw0, f"dw acc={int(accumulate_dw)}")


# ------------------------------------------------------------------------------------------------ argument rejection
def _rejected(call, outputs, name):
    """`call()` must fail before any launch: every pre-filled output keeps its bits."""
    from yat_amd import lib as L
    before = [o.clone() for o in outputs]
    with pytest.raises(L.YatLibraryError):
        call()
    torch.cuda.synchronize()
    for i, (o, b) in enumerate(zip(outputs, before)):
        same(o, b, f"{name} output {i} after the rejected call")


def test_rejects_what_the_kernels_cannot_serve(ops):
    """D off a multiple of 8 or beyond 4096, a leading dimension off a multiple of 8 or below nseg * D, three segments, null
    operands, one weight gradient of two: YAT_EINVAL with no launch."""
    M, EINVAL = 4, -1
    ws = wspace(1 << 20)

    def operands(D, nseg, ld):
        W = nseg * D
        wide = lambda seed: rnd(M, ld, seed=seed)[:, :W]                                   # noqa: E731
        return dict(x=wide(1), dy=wide(2), y=wide(3), dx=wide(4), w=[rnd(D, seed=5 + s) for s in range(nseg)],
                    dw=[rnd(D, seed=8 + s) for s in range(nseg)], rstd=torch.full((M, nseg), 0.5, device=DEV))

    def both(o, name):
        _rejected(lambda: ops.rmsnorm_seg_fwd(o["x"], o["w"], EPS, o["y"], o["rstd"]), [o["y"], o["rstd"]], f"fwd {name}")
        _rejected(lambda: ops.rmsnorm_seg_bwd(o["x"], o["w"], o["rstd"], o["dy"], o["dx"], o["dw"], ws), [o["dx"], *o["dw"]],
                  f"bwd {name}")
    both(operands(12, 2, 40), "D=12")
    both(operands(4104, 1, 4104), "D=4104")
    both(operands(64, 2, 132), "ld=132")                       # ld % 8
    both(operands(64, 3, 192), "nseg=3")
    o = operands(64, 2, 128)
    narrow = lambda t: t.as_strided((M, 128), (64, 1))                                      # noqa: E731  (ld < nseg * D)
    both({**o, "x": narrow(o["x"])}, "ldx < nseg * D")
    _rejected(lambda: ops.rmsnorm_seg_fwd(o["x"], o["w"], EPS, narrow(o["y"]), o["rstd"]), [o["y"], o["rstd"]], "fwd ldy < nseg * D")
    _rejected(lambda: ops.rmsnorm_seg_bwd(o["x"], o["w"], o["rstd"], narrow(o["dy"]), o["dx"], o["dw"], ws), [o["dx"], *o["dw"]],
              "bwd lddy < nseg * D")
    _rejected(lambda: ops.rmsnorm_seg_bwd(o["x"], o["w"], o["rstd"], o["dy"], narrow(o["dx"]), o["dw"], ws), [o["dx"], *o["dw"]],
              "bwd lddx < nseg * D")
    _rejected(lambda: ops.rmsnorm_seg_bwd(o["x"], o["w"], o["rstd"], o["dy"], o["dx"], o["dw"], None), [o["dx"], *o["dw"]],
              "bwd dw without a workspace")
    # null operands and one weight gradient of two: straight at the C ABI (the wrapper would not build such a call)
    lib, p, st = ops._lib(), ops._p, ops._stream()
    before = [t.clone() for t in (o["y"], o["dx"], o["rstd"], *o["dw"])]
    fwd = [M, 64, 2, EPS, p(o["x"]), 128, p(o["w"][0]), p(o["w"][1]), p(o["y"]), 128, None, p(o["rstd"]), st]
    for i in (4, 6, 7, 8, 11):
        assert lib.yat_rmsnorm_seg_fwd(*[None if j == i else a for j, a in enumerate(fwd)]) == EINVAL, i
    bwd = [M, 64, 2, p(o["x"]), 128, p(o["w"][0]), p(o["w"][1]), p(o["rstd"]), p(o["dy"]), 128, p(o["dx"]), 128, p(o["dw"][0]),
           p(o["dw"][1]), 0, p(ws), st]
    for i in (3, 5, 6, 7, 8, 10, 12, 13):
        assert lib.yat_rmsnorm_seg_bwd(*[None if j == i else a for j, a in enumerate(bwd)]) == EINVAL, i
    torch.cuda.synchronize()
    for t, b in zip((o["y"], o["dx"], o["rstd"], *o["dw"]), before):
        same(t, b, "outputs after the null-operand calls")
