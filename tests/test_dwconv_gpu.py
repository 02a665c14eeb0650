"""The GLU depthwise convolution (csrc/dwconv_glu.hip, csrc/dwconv_tile.hpp: the streaming forward, the five band kernels, the
three direct kernels, dwconv_reduce_kernel) held to exact sums at every walk, band and edge -- GPU.

tests/dwconv_ref.py holds the table, plan() (which kernel and geometry a shape takes), the inputs and the fp64 model;
test_dwconv_ref_cpu.py shows that the table reaches every class and that the check reports each of eleven planted errors.
Inputs are small integers for which every sum a kernel forms is exact in fp32 in any order (asserted: the model's largest sum
of |terms| stays below 2^24) and the library's sigmoid is exactly 1 or exactly 0 (asserted: test_library_silu_is_exact), so
every comparison with the model is torch.equal after + 0.0.  Per case, built once:
forward      with and without u_out: y identical, u and y equal the model
backward     with dy: the du pass 1 leaves at the head of the workspace, dz, dwdw and dbdw equal the model
backward     through du= with dz_colsum, accumulate off and then on (onto integer-valued contents): all four equal the model
guards       every output is a window inside a larger buffer, one image row of 2 Hc channels of a fixed finite bit pattern on
             either side, bit-identical after each call (the range-checked buffer stores answer for that)
One real-valued forward (rnd data, the fp64 model with the kernels' rounding points, close() at its default tolerance) runs on
the multi-step streaming cases, so that the rounding of u before the GLU is seen at nsteps > 1 as well.
"""
import types

import pytest
import torch
import torch.nn.functional as F

from tests import dwconv_ref as R
from tests.gpu_common import BF, DEV, _FAILS, _collect_failures, close, rnd  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


@pytest.fixture(scope="module", params=R.TABLE, ids=lambda c: c.name)
def built(request):
    case = request.param
    inp = R.build(case.dims, DEV, seed=2)
    m = R.model(case.dims, inp)
    for name, bound in m.bounds.items():
        assert bound < R.EXACT_LIMIT, (case.name, name, bound)
    yield types.SimpleNamespace(case=case, dims=case.dims, inp=inp, m=m)
    torch.cuda.empty_cache()


def _check(b, name, got, want):
    fails = R.check(b.dims, f"{b.case.name} {name}", got, want)
    for f in fails:
        print(f"[dwconv exact] {f}")
    _FAILS.extend(fails)


def _untouched(b, name, win):
    if not (win.guards_intact() and bool((win.view.view(torch.int16) == R.GUARD_BITS).all())):
        _FAILS.append(f"{b.case.name} {name}: written although not passed")


def test_library_silu_is_exact(ops):
    """sigmoid_f is exactly 1 on the live ranges and exactly 0 on the dead ones: SiLU(x) = x or +-0, SiLU'(x) = 1 or +-0"""
    for lo, hi, live in ((*R.Z_LIVE, True), (R.G_LIVE - 50, R.G_LIVE + 50, True), (*R.Z_DEAD, False),
                         (R.G_DEAD - 50, R.G_DEAD + 50, False)):
        x = torch.arange(lo, hi + 1, dtype=torch.float32).to(BF).to(DEV)
        assert torch.equal(x.float().cpu(), torch.arange(lo, hi + 1, dtype=torch.float32))
        y, dx = ops.act_fwd(x, "silu"), ops.act_bwd(x, torch.ones_like(x), "silu")
        print(f"[dwconv exact] silu on [{lo}, {hi}]: {sorted(set((y.float() - (x.float() if live else 0)).tolist()))} off, "
              f"silu' {sorted(set(dx.float().tolist()))}")
        assert torch.equal(y.float() + 0.0, x.float() if live else torch.zeros_like(x, dtype=torch.float32))
        assert torch.equal(dx.float() + 0.0, torch.full_like(x, 1.0 if live else 0.0, dtype=torch.float32))


def test_forward(ops, built):
    b, inp, m = built, built.inp, built.m
    W0, W1 = R.windows(b.dims, DEV, ("y", "u")), R.windows(b.dims, DEV, ("y", "u"))
    ops.dwconv_glu_fwd(inp.s, *b.dims, inp.wdw, inp.bdw, W0["y"].view)
    ops.dwconv_glu_fwd(inp.s, *b.dims, inp.wdw, inp.bdw, W1["y"].view, u_out=W1["u"].view)
    torch.cuda.synchronize()
    if not torch.equal(W0["y"].buf.view(torch.int16), W1["y"].buf.view(torch.int16)):
        _FAILS.append(f"{b.case.name}: y differs with u_out")
    _untouched(b, "u", W0["u"])
    _check(b, "y (no u_out)", W0["y"], m.y)
    _check(b, "y", W1["y"], m.y)
    _check(b, "u", W1["u"], m.u)


def _workspace(ops, dims):
    return torch.full((ops.dwconv_glu_bwd_workspace_bytes(*dims),), 0x4B, dtype=torch.uint8, device=DEV)


def test_backward_from_dy(ops, built):
    b, inp, m = built, built.inp, built.m
    M, C2 = b.dims[0] * b.dims[1] * b.dims[2], 2 * b.dims[3]
    W = R.windows(b.dims, DEV, ("dz", "dw", "db", "dzs"))
    ws = _workspace(ops, b.dims)
    ops.dwconv_glu_bwd(inp.s, inp.z, *b.dims, inp.wdw, inp.bdw, inp.dy, W["dz"].view, W["dw"].view, W["db"].view, ws)
    torch.cuda.synchronize()
    _check(b, "du (pass 1, workspace)", ws[:M * C2 * 2].view(BF).view(M, C2), m.du1)
    _check(b, "dz", W["dz"], m.dz1)
    _check(b, "dwdw", W["dw"], m.dw1)
    _check(b, "dbdw", W["db"], m.db1)
    _untouched(b, "dz_colsum", W["dzs"])


def test_backward_through_du(ops, built):
    b, inp, m = built, built.inp, built.m
    ws = _workspace(ops, b.dims)
    prev = dict(dw=inp.prev_dw, db=inp.prev_db, dzs=inp.prev_dzs)
    for acc, want in ((False, m.plain), (True, m.accum)):
        W = R.windows(b.dims, DEV, ("dz", "dw", "db", "dzs"), prev=prev if acc else None)
        ops.dwconv_glu_bwd(inp.s, inp.z, *b.dims, inp.wdw, inp.bdw, None, W["dz"].view, W["dw"].view, W["db"].view, ws,
                           accumulate=acc, dz_colsum=W["dzs"].view, du=inp.du)
        torch.cuda.synchronize()
        tag = "accumulate" if acc else "du="
        _check(b, f"dz ({tag})", W["dz"], m.dz2)
        _check(b, f"dwdw ({tag})", W["dw"], want["dw"])
        _check(b, f"dbdw ({tag})", W["db"], want["db"])
        _check(b, f"dz_colsum ({tag})", W["dzs"], want["dzs"])


@pytest.mark.parametrize("case", R.STREAM_MULTI, ids=lambda c: c.name)
def test_forward_real_valued_multi_step(ops, case):
    """rnd data through the streaming forward at nsteps > 1 against the fp64 model rounded where the kernel rounds: s, u,
    SiLU(ug) and y"""
    B, h, w, Hc = case.dims
    assert max(R.plan(*case.dims)["fwd"]["steps"]) >= 3
    M = B * h * w
    z = rnd(M, 2 * Hc, seed=71)
    wdw, bdw = rnd(2 * Hc, 9, scale=1 / 3, seed=72), rnd(2 * Hc, scale=0.1, seed=73)
    s_act = F.silu(z.float()).to(BF)
    W = R.windows(case.dims, DEV, ("y", "u"))
    ops.dwconv_glu_fwd(s_act, B, h, w, Hc, wdw, bdw, W["y"].view, u_out=W["u"].view)
    u, y, _, _ = R.model_fwd(case.dims, s_act, wdw, bdw, sigmoid=torch.sigmoid)
    close(W["u"].view, u, f"dwconv_u real {case.name}")
    close(W["y"].view, y, f"dwconv_fwd real {case.name}")
    assert W["y"].guards_intact() and W["u"].guards_intact()
