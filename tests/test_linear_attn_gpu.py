"""ReLU linear attention (csrc/linear_attn.hip: la_state_kernel, la_fwd_kernel, la_bwd_q_kernel, la_reduce_slabs_kernel,
la_bwd_kv_kernel) at every token class, grid total, stride and dead row -- GPU.

Inputs, the fp64 truth and the flow (the diffusers processor's own arithmetic: fp32, rounded to bf16) come from
tests/linear_attn_ref.py, computed once per case on the CPU.  test_linear_attn_ref_cpu.py holds a torch emulation of the
kernels' arithmetic to the same conditions, and shows that the emulation without the lo halves violates them.

Parity (linear_attn_ref.conditions), per head and per tensor (out, dq, dk, dv), into outputs that start as NaN and with
a workspace that starts as 0xFF bytes:
(a) finite everywhere (so every unit of the remapped grid was produced); exactly zero on the dead heads of `sparse`;
(b) as_good_as(hip, flow, truth), the helper's own slack and floor;
(c) flips <= 0.01 * numel + 2 for the kinds randn, sparse, zeros, where a flip is an element whose bits differ from the
    correctly rounded fp64 result.  The hi + lo split carries S, dU and dS to <= 2^-17 relative and bf16 values are spaced
    >= 2^-8 relative, so a result lands on the other side of a rounding boundary with probability <~ 2^-8 = 0.4 % where
    the sums do not cancel; the emulation's worst is 0.39 % (dq of `sparse`, where the fp32 flow flips 0.34 % itself).
    With every lo half dropped the emulation flips >= 4 % of each tensor.  bf16 rounding (1.65e-3 relative L2) hides that loss
    from a norm: the hi-only forward scores 1.9e-3.
    At N = 1 the state has rank one and dq = dk = 0 in exact arithmetic, so (b) and (c) have no truth to measure against on
    those two tensors: there |result| <= 2^-15 of the sum of the |terms| that cancel (derived in linear_attn_ref.conditions).
(d) `offset` (q, k x 4, v + 3) has no flip cap: dq = dU S + S[32] dU32 cancels, and the arithmetic the kernel's header
    describes flips more the larger N is.  Fraction of elements that are not the correctly rounded fp64 result, (B, H) =
    (1, 3) at N = 4096 and (2, 3) below, kernel on an MI355X / emulation / flow:
        N       dq, %                     dk, %                    dv, %
        17       1.65 /  1.65 / 0.09      0.74 / 0.77 / 0.06       0.43 / 0.43 / 0.00
        257      4.26 /  4.28 / 0.27      0.53 / 0.55 / 0.04       0.26 / 0.26 / 0.01
        1020     7.33 /  7.31 / 0.47      0.58 / 0.61 / 0.06       0.29 / 0.28 / 0.01
        4096    11.85 / 11.80 / 0.88      0.50 / 0.55 / 0.05       0.22 / 0.23 / 0.02
    The kernel does what the emulation does.  (b) holds: at N = 4096 the kernel's dq is 1.777e-3 from the truth in relative
    L2 and the flow's 1.655e-3 (1.681e-3 and 1.649e-3 at N = 1020); dk and dv sit where the flow sits (1.659e-3, 1.658e-3).
    The test prints all three rates whenever it runs.

Layouts: q | v | pad | k | pad inputs, `out` as a column slice, padded dout and dqkv, and a row slice of a batch give the
packed call's bits and leave every other byte (0x7FC1 canaries) as it was.
No hidden state: repeated calls, a poisoned workspace and single images give the batch's bits.
"""
import pytest
import torch

from tests import linear_attn_ref as R
from tests.gpu_common import BF, DEV, _FAILS, _collect_failures, as_good_as, close, rel  # noqa: F401  (autouse fixture)

pytestmark = pytest.mark.gpu

TOKEN_CLASSES = [(2, n, 3) for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1020, 1025)]
GRID_TOTALS = [(1, 40, 1), (1, 40, 3), (1, 40, 7), (1, 300, 4), (3, 257, 3), (1, 40, 36), (1, 40, 70), (1, 600, 5)]
SHAPES = TOKEN_CLASSES + GRID_TOTALS + [(1, 4096, 3)]
FEW = [(2, 17, 3), (2, 257, 3), (2, 1020, 3), (1, 4096, 3)]
CASES = ([(k, *s) for s in SHAPES for k in ("randn", "sparse")]
         + [(k, *s) for s in FEW for k in ("zeros", "offset")])
CANARY = 0x7FC1                  # a bf16 NaN no kernel produces


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


def _state_floats(B, H):
    return B * H * 33 * 32


def _ws(ops, B, N, H, fill=0xFF):
    return torch.full((ops.linear_attn_workspace_bytes(B, N, H),), fill, dtype=torch.uint8, device=DEV)


def _canary(rows, cols):
    return torch.full((rows, cols), CANARY, dtype=torch.int16, device=DEV).view(BF)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def same(a, b, name):
    if a.shape != b.shape or not torch.equal(_bits(a), _bits(b)):
        _FAILS.append(f"{name}: not bit-identical")
        print(f"[parity] {name}: NOT BIT-IDENTICAL")


def _packed(ops, qkv, dout, B, N, H, state="own", ws_fill=0xFF):
    """forward + backward on the packed layout into NaN outputs; state = "own": the backward recomputes S,
    "given": it gets the forward's.  Returns out, dqkv and the forward's state (device tensors)."""
    D = 32 * H
    out = torch.full((B * N, D), float("nan"), dtype=BF, device=DEV)
    dqkv = torch.full((B * N, 3 * D), float("nan"), dtype=BF, device=DEV)
    ws = _ws(ops, B, N, H, ws_fill)
    ops.linear_attn_fwd(qkv, B, N, H, D, 2 * D, out, ws)
    st = ws.view(torch.float32)[:_state_floats(B, H)].clone()
    ws = _ws(ops, B, N, H, ws_fill)                       # with state= the workspace's own S region holds NaN
    ops.linear_attn_bwd(qkv, B, N, H, D, 2 * D, dout, dqkv, ws, state=st if state == "given" else None)
    return out, dqkv, st


def _got(out, dqkv, D):
    out, dqkv = out.cpu(), dqkv.cpu()
    return {"out": out, "dq": dqkv[:, :D], "dk": dqkv[:, D:2 * D], "dv": dqkv[:, 2 * D:]}


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("kind,B,N,H", CASES)
def test_linear_attn_parity(ops, kind, B, N, H):
    c = R.case(kind, B, N, H)
    D = 32 * H
    out, dqkv, _ = _packed(ops, c["qkv"].to(DEV), c["dout"].to(DEV), B, N, H)
    got = _got(out, dqkv, D)
    R.conditions(got, c, f"linattn {kind} B={B} N={N} H={H}", flip_cap=kind != "offset")
    if kind == "offset":
        mine, flow = R.flip_rates(got, c), R.flip_rates(c["flow"], c)
        emu = R.flip_rates(dict(zip(("out", "dq", "dk", "dv"), R.emulate(c["qkv"], c["dout"], B, N, H, D, 2 * D))), c)
        for n in ("out", "dq", "dk", "dv"):
            print(f"[flips] offset N={N} {n}: kernel {100 * mine[n]:.2f} %  emulation {100 * emu[n]:.2f} %  flow {100 * flow[n]:.2f} %"
                  f"  rel l2 kernel {rel(got[n], c['truth'][n]):.3e} flow {rel(c['flow'][n], c['truth'][n]):.3e}")


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("B,N,H", [(2, 257, 3), (1, 1020, 3)])
def test_linear_attn_strided_layout(ops, B, N, H):
    """q | v | pad | k | pad rows, `out` in the right half of a wider buffer, padded dout and dqkv: the packed call's bits in
    the written ranges, the canary everywhere else, inputs untouched."""
    c = R.case("randn", B, N, H)
    D, M = 32 * H, B * N
    qkv, dout = c["qkv"].to(DEV), c["dout"].to(DEV)
    out0, dqkv0, _ = _packed(ops, qkv, dout, B, N, H)
    k_off, v_off = 2 * D + 8, D
    wide = _canary(M, 3 * D + 24)
    wide[:, :D], wide[:, k_off:k_off + D], wide[:, v_off:v_off + D] = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    obuf, dobuf, dbuf = _canary(M, 2 * D + 8), _canary(M, D + 16), _canary(M, 3 * D + 64)
    dobuf[:, :D] = dout
    wide_in, dobuf_in = wide.clone(), dobuf.clone()
    ws = _ws(ops, B, N, H)
    ops.linear_attn_fwd(wide, B, N, H, k_off, v_off, obuf[:, D + 8:], ws)
    ops.linear_attn_bwd(wide, B, N, H, k_off, v_off, dobuf[:, :D], dbuf, _ws(ops, B, N, H))
    same(obuf[:, D + 8:], out0, "strided out")
    same(obuf[:, :D + 8], _canary(M, D + 8), "strided out: columns left of the slice")
    same(dbuf[:, :D], dqkv0[:, :D], "strided dq")
    same(dbuf[:, k_off:k_off + D], dqkv0[:, D:2 * D], "strided dk")
    same(dbuf[:, v_off:v_off + D], dqkv0[:, 2 * D:], "strided dv")
    same(dbuf[:, 2 * D:k_off], _canary(M, 8), "strided dqkv: pad between dv and dk")
    same(dbuf[:, k_off + D:], _canary(M, 3 * D + 64 - k_off - D), "strided dqkv: pad after dk")
    same(wide, wide_in, "strided qkv (input)")
    same(dobuf, dobuf_in, "strided dout (input)")


def test_linear_attn_row_slice(ops):
    """images 1 .. B-1 of a batch of 3, called with B - 1 on row slices: the batch's bits, image 0's rows untouched"""
    B, N, H = 3, 257, 3
    c = R.case("randn", B, N, H)
    D = 32 * H
    qkv, dout = c["qkv"].to(DEV), c["dout"].to(DEV)
    out0, dqkv0, _ = _packed(ops, qkv, dout, B, N, H)
    obuf, dbuf = _canary(B * N, D), _canary(B * N, 3 * D)
    ops.linear_attn_fwd(qkv[N:], B - 1, N, H, D, 2 * D, obuf[N:], _ws(ops, B - 1, N, H))
    ops.linear_attn_bwd(qkv[N:], B - 1, N, H, D, 2 * D, dout[N:], dbuf[N:], _ws(ops, B - 1, N, H))
    same(obuf[N:], out0[N:], "row slice out")
    same(dbuf[N:], dqkv0[N:], "row slice dqkv")
    same(obuf[:N], _canary(N, D), "row slice out: image 0")
    same(dbuf[:N], _canary(N, 3 * D), "row slice dqkv: image 0")


# ------------------------------------------------------------------------------------------------ no hidden state
@pytest.mark.parametrize("B,N,H", [(2, 257, 3), (1, 1025, 5)])
def test_linear_attn_no_hidden_state(ops, B, N, H):
    c = R.case("randn", B, N, H)
    D = 32 * H
    qkv, dout = c["qkv"].to(DEV), c["dout"].to(DEV)
    out0, dq_own, st = _packed(ops, qkv, dout, B, N, H, state="own")
    st_in = st.clone()
    for state in ("own", "given"):
        for fill in (0xFF, 0x00):                          # twice each: a repeat, and a poisoned against a zeroed workspace
            for rep in range(2):
                out, dqkv, st2 = _packed(ops, qkv, dout, B, N, H, state=state, ws_fill=fill)
                tag = f"state={state} workspace={fill:#04x} run {rep}"
                same(out, out0, f"out {tag}")
                same(dqkv, dq_own, f"dqkv {tag}")
                same(st2.view(torch.int32), st_in.view(torch.int32), f"forward state {tag}")
    dqkv = torch.full_like(dq_own, float("nan"))
    ops.linear_attn_bwd(qkv, B, N, H, D, 2 * D, dout, dqkv, _ws(ops, B, N, H), state=st)
    same(st.view(torch.int32), st_in.view(torch.int32), "state= tensor after the backward")
    same(dqkv, dq_own, "dqkv from the kept state")
    for b in range(B):                                     # each image alone, forward and both backwards
        rows = slice(b * N, (b + 1) * N)
        for state in ("own", "given"):
            out, dqkv, _ = _packed(ops, qkv[rows], dout[rows], 1, N, H, state=state)
            same(out, out0[rows], f"out image {b} alone ({state} state)")
            same(dqkv, dq_own[rows], f"dqkv image {b} alone ({state} state)")
