"""The GEMM family (csrc/gemm.hip, csrc/gemm256.hip) at every leading dimension and narrow edge -- GPU.

tests/gemm_ref.py holds the case table: every operand is a view into a larger buffer (inputs NaN outside the view, outputs one
signalling-NaN bit pattern everywhere), in all four layouts, on the 128 x 128 kernel, both 256-row tiles, both split-K paths
and the policy's own pick; N % 8 == 4 and leading dimensions of 4 (mod 8) put the 256-row kernels on their per-lane 8-byte
epilogue.  Per case, one launch on the views and one on the contiguous twin, then

  * check(): nothing outside the output windows was written, no input was modified, and the window is bit-identical to the
    contiguous launch -- both epilogues and every stride do the same fp32 arithmetic with the same rounding points;
  * close(window, model) with the tolerances test_kernels_gpu.py states (the bias gradient a_rowsum_out: the bounds
    test_gemm_skinny_long_k holds it to).  The stages behind an aux_out copy start from the launch's own copy, as in
    test_gemm256_second_operand_pair.

test_gemm_layout_cpu.py shows, without a GPU, that the table reaches every class and that these conditions catch a store past
N or M, a swapped leading dimension, a read past an operand's width, a dropped K tail and a wrong gate row.
"""
import pytest
import torch

from tests import gemm_ref as R
from tests.gpu_common import _FAILS, _collect_failures, close  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


def _launch(ops, case, v):
    kw = {}
    if "bias" in v:
        kw["bias"] = v["bias"]
    if "aux" in v:
        kw.update(aux_out=v["aux"], ld_aux=v["aux"].stride(0))
    if case.res is not None:
        kw.update(residual=v["res"], ld_residual=v["res"].stride(0))
    if case.gate is not None:
        kw.update(gate=v["gate"], ld_gate=v["gate"].stride(0) if v["gate"].dim() == 2 else 0, rows_per_batch=case.gate[1])
    if case.rowsum is not None:
        kw.update(a_rowsum=v["rowsum"], a_rowsum_accumulate=case.rowsum == "acc")
    ops.gemm(v["a"], v["b"], v["c"], a_t=bool(case.a_t), b_t=bool(case.b_t), M=case.M, N=case.N, K=case.K,
             lda=v["a"].stride(0), ldb=v["b"].stride(0), ldc=v["c"].stride(0), variant=case.path, activation=case.act,
             pre_add=v.get("pre"), dact_z=v.get("dact"), glu_u=v.get("glu"), **kw)


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_gemm_placement(ops, case):
    before, twin = R.build(case, seed=1 + R.TABLE.index(case))
    dev, tdev = {k: t.to(DEV) for k, t in before.items()}, {k: t.to(DEV) for k, t in twin.items()}
    _launch(ops, case, R.views(case, dev))
    _launch(ops, case, R.twin_views(case, tdev))
    torch.cuda.synchronize()
    after, twin_out = {k: t.cpu() for k, t in dev.items()}, {k: t.cpu() for k, t in tdev.items()}
    _FAILS.extend(R.check(case, before, after, twin_out))
    got = R.views(case, after)
    for name, want in R.model(case, R.views(case, before), own=got.get("aux")).items():
        if name == "rowsum":
            close(got[name], want, f"{case.name} {name}", tol=4e-3, ulps=3.0)
        else:
            close(got[name], want, f"{case.name} {name}")


def _sentinel(*shape):
    return R._sentinel(*shape).to(DEV)


def _untouched(t):
    return bool((R.bits(t.cpu()) == R.bits(R._sentinel(1))[0]).all())


def test_gemm_grouped_placement(ops):
    """ops.wgrad_grouped on column slices: dy and x are slices of wider NaN-padded buffers, each out is the first N rows of a
    taller buffer, each bias gradient sits in a longer vector.  Plain and accumulating, every result is bit-identical to the
    single launch on the 256 x 256 tile with the same strides, and nothing around the outputs is written."""
    g = torch.Generator(device="cpu").manual_seed(7)
    items, singles, keep = [], [], []
    for T, N, K in R.GROUPED:
        dyb, xb = torch.full((T + 2, N + 24), float("nan"), dtype=BF), torch.full((T + 2, K + 40), float("nan"), dtype=BF)
        dyb[1:1 + T, 8:8 + N] = (torch.randn(T, N, generator=g) * T ** -0.5).to(BF)
        xb[1:1 + T, 16:16 + K] = torch.randn(T, K, generator=g).to(BF)
        dyd, xd = dyb.to(DEV), xb.to(DEV)
        dy, x = dyd[1:1 + T, 8:8 + N], xd[1:1 + T, 16:16 + K]
        outs = [(_sentinel(N + 3, K), _sentinel(3 + N + 5)) for _ in range(2)]
        items.append((dy, x, outs[0][0][:N], outs[0][1][3:3 + N]))
        singles.append((dy, x, outs[1][0][:N], outs[1][1][3:3 + N]))
        keep.append((dyb, xb, dyd, xd, outs))
    for accumulate in (False, True):
        ops.wgrad_grouped(items, accumulate=accumulate)
        for dy, x, out, db in singles:
            T, (N, K) = dy.shape[0], out.shape
            ops.gemm(dy, x, out, a_t=True, b_t=True, M=N, N=K, K=T, lda=dy.stride(0), ldb=x.stride(0), ldc=K, variant=4,
                     residual=out if accumulate else None, a_rowsum=db, a_rowsum_accumulate=accumulate)
        torch.cuda.synchronize()
        for (dy, x, out, db), (_, _, out1, db1), (dyb, xb, dyd, xd, outs), sh in zip(items, singles, keep, R.GROUPED):
            tag = f"grouped{'_acc' if accumulate else ''} {sh}"
            N = out.shape[0]
            if not (torch.equal(out, out1) and torch.equal(db, db1)):
                _FAILS.append(f"{tag}: differs from the single launch")
            for full, vec in outs:
                if not (_untouched(full[N:]) and _untouched(vec[:3]) and _untouched(vec[3 + N:])):
                    _FAILS.append(f"{tag}: guard: written outside the output window")
            if not (torch.equal(R.bits(dyd.cpu()), R.bits(dyb)) and torch.equal(R.bits(xd.cpu()), R.bits(xb))):
                _FAILS.append(f"{tag}: an input was modified")
            ref, refb = dy.float().cpu().double().T @ x.float().cpu().double(), dy.float().cpu().double().sum(0)
            if accumulate:
                ref, refb = R.rb(ref.float()) + R.rb(ref.float()), R.rb(refb.float()) + R.rb(refb.float())
            close(out.cpu(), ref.float().to(BF), tag)
            close(db.cpu(), refb.float().to(BF), tag + " bias gradient", tol=4e-3, ulps=3.0)


# what the entry point refuses: (name, arguments that differ from a valid 64 x 64 x 64 launch)
REJECTED = (
    ("N % 4", dict(N=62)),
    ("lda % 8", dict(lda=68)),
    ("ldb % 8", dict(ldb=68)),
    ("ldc % 4", dict(ldc=66)),
    ("a_t with M % 8", dict(a_t=True, b_t=True, M=60)),
    ("b_t with N % 8", dict(b_t=True, N=60)),
    ("K % 8, A and B k-contiguous", dict(K=60)),
    ("K % 8, A k-contiguous", dict(b_t=True, K=60)),
    ("K % 8, B k-contiguous", dict(a_t=True, K=60)),
    ("split-K with N % 8 == 4", dict(N=60, variant=204)),
    ("split-K with ldc % 8 == 4", dict(ldc=68, variant=204)),
    ("glu_u with ld_glu_u % 8 == 4", dict(b_t=True, variant=4, glu=132)),
    ("dact_z on the 128 x 128 kernel", dict(b_t=True, variant=1, dact=64)),
    ("lda < K", dict(lda=56)),
    ("ldb < K", dict(ldb=56)),
    ("lda < M, A k-strided", dict(a_t=True, b_t=True, lda=56)),
    ("ldb < N, B k-strided", dict(b_t=True, ldb=56)),
    ("ldc < N", dict(ldc=56)),
    ("ld_residual < N", dict(res=56)),
    ("ld_aux < N", dict(aux=56)),
    ("ld_pre_add < N", dict(pre=56)),
    ("ld_dact_z < N", dict(b_t=True, variant=4, dact=56)),
    ("ld_glu_u < 2N", dict(b_t=True, variant=4, glu=120)),
)


@pytest.mark.parametrize("what,args", REJECTED, ids=[r[0] for r in REJECTED])
def test_gemm_rejects(ops, what, args):
    """Every refused call raises before any launch: the output, filled with the sentinel, is untouched."""
    from yat_amd.lib import YatLibraryError
    args = dict(args)
    g = torch.Generator(device="cpu").manual_seed(3)
    a, b = (torch.randn(128, 128, generator=g).to(BF).to(DEV) for _ in range(2))
    out, aux = _sentinel(128, 256), _sentinel(128, 128)
    kw = dict(a_t=False, b_t=False, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, variant=0)
    for name in ("res", "aux", "pre", "dact", "glu"):
        if name in args:
            ld = args.pop(name)
            t = torch.zeros(128 * 256, dtype=BF, device=DEV)[:64 * ld].view(64, ld)
            if name == "res":
                kw.update(residual=t, ld_residual=ld)
            elif name == "aux":
                kw.update(aux_out=aux, ld_aux=ld)
            else:
                kw.update({"pre": dict(pre_add=t), "dact": dict(dact_z=t, activation="silu"), "glu": dict(glu_u=t, ldc=128)}[name])
    kw.update(args)
    with pytest.raises(YatLibraryError):
        ops.gemm(a, b, out, **kw)
    torch.cuda.synchronize()
    assert _untouched(out) and _untouched(aux), what


def test_gemm_grouped_rejects(ops):
    """The grouped entry point shares the argument checks: a dy whose row stride is below its width is refused."""
    from yat_amd.lib import YatLibraryError
    dy, x = torch.zeros(64, 64, dtype=BF, device=DEV), torch.zeros(64, 64, dtype=BF, device=DEV)
    out = _sentinel(64, 64)
    with pytest.raises(YatLibraryError):
        ops.wgrad_grouped([(torch.as_strided(dy, (64, 64), (56, 1)), x, out)])
    torch.cuda.synchronize()
    assert _untouched(out)
