"""Softmax attention (csrc/sdpa.hip: sdpa_fwd_kernel, sdpa_bwd_dq_kernel, sdpa_bwd_dkv_kernel) held to exact results at every
dispatch class, ragged edge and stride -- GPU.

Inputs, the plain fp64 reference and the case lists come from tests/sdpa_selector_ref.py (selector inputs: softmax weights
exactly 1/g or 0, every product and sum exact in fp32, so the kernels must store the bits the reference rounds to);
test_sdpa_selector_ref_cpu.py proves those properties and that the lists reach every instantiation the host can select.

Every case runs the forward twice (dense v in [-8, 8], then the sparse -1 / 0 / 1 v of the backward), the backward once with parts = 3 on the dense grid and, where there is a key bias, again with
the work list, then all of that on packed keys, and asserts ``torch.equal`` against the expectation for out, delta, dq,
dk and dv.  Nothing is compared with another run of the kernels.
  * Every operand lives in a buffer of its own, at a nonzero row and a nonzero column, with leading dimensions that all
    differ and exceed H * dh, at the finest alignment include/yat_hip.h allows (8 elements for ldq, ldkv, lddo and the
    backward's ldo; 4 for the forward's ldo, lddq and lddkv).  Output buffers start as a canary (bf16 bits 0x7FC1) and are
    compared whole, so a write outside the tensor's rows and columns fails; input guards hold 32768, which would wreck a
    score, an output or a gradient if read as data.
  * dK / dV rows of masked keys are exact zeros in the padded layout (part of the expectation); rows of no image in the
    packed layout keep the canary.  -0 and +0 count as equal (the dK store multiplies by -scale), everything else by bits.
  * lse: rows with one winner equal the winner's scaled score exactly (log 1 = 0); rows with 2 or 4 winners lie within
    2 fp32 ulps, at their magnitude, of fp32(score + ln g) from the fp64 reference.  Measured on an MI355X: 0 ulps in every
    case -- the row sum is exactly g and the hardware logarithm of 2 and 4 gives the correctly rounded sum (the largest
    distance is printed per case).
"""
import pytest
import torch

from tests import sdpa_selector_ref as R
from tests.gpu_common import BF, DEV

pytestmark = pytest.mark.gpu

CANARY = 0x7FC1                  # a bf16 NaN no kernel produces
GUARD = 32768.0                  # input guard rows and columns: finite, exact in bf16, ruinous if read as data
# (columns beyond H * dh, first column, rows before, rows after) per operand: every leading dimension differs
# (pads and first columns are 8 mod 16 where the interface asks for multiples of 8, and 4 mod 8 where it asks for 4)
LAYOUT = dict(q=(24, 8, 1, 2), k=(40, 8, 2, 1), v=(40, 24, 1, 3), out_fwd=(12, 4, 2, 1), out_bwd=(56, 8, 1, 1),
              dout=(72, 24, 3, 1), dq=(20, 4, 1, 2), dk=(28, 12, 2, 2), dv=(28, 4, 1, 1))
assert len({LAYOUT[n][0] for n in ("q", "k", "out_fwd", "out_bwd", "dout", "dq", "dk")}) == 7


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


def _window(name, rows, D, data=None):
    """(buffer, view [rows, D]): ``data`` inside input guards, or canaries to be written by a kernel"""
    pad, c0, r0, r1 = LAYOUT[name]
    if data is None:
        buf = torch.full((r0 + rows + r1, D + pad), CANARY, dtype=torch.int16, device=DEV).view(BF)
    else:
        buf = torch.full((r0 + rows + r1, D + pad), GUARD, dtype=BF, device=DEV)
        buf[r0:r0 + rows, c0:c0 + D] = data.to(DEV)
    return buf, buf[r0:r0 + rows, c0:c0 + D]


def _whole(name, rows, D, expected, keep=None):
    """the bits of a whole output buffer: canaries around ``expected`` (rows ``keep``: only those rows are written)"""
    buf, view = _window(name, rows, D)
    if keep is None:
        view.copy_(expected.to(DEV))
    else:
        view[keep.to(DEV)] = expected.to(DEV)
    return _bits(buf)


def _bits(buf):
    """bf16 bits with -0 folded onto +0: the two compare equal, as they do under torch.equal on values"""
    b = buf.view(torch.int16)
    return torch.where(b == -32768, torch.zeros_like(b), b)


def _check(fails, what, buf, want):
    got = _bits(buf)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, c = bad[0].tolist()
        fails.append(f"{what}: {bad.shape[0]} elements differ, first at buffer (row, col) ({r}, {c}): bits "
                     f"{got[r, c].item() & 0xffff:#06x}, expected {want[r, c].item() & 0xffff:#06x}")


def _check_lse(fails, what, lse, exp):
    lse, want, one = lse.cpu(), exp["lse"], exp["one_winner"]
    if not torch.equal(lse[one], want[one]):
        fails.append(f"{what}: lse of a row with one winner is not its score")
    dist = ((lse.double() - want.double()).abs() / R.ulp32(want)).max().item()
    if not dist <= 2:
        fails.append(f"{what}: lse {dist:.2f} fp32 ulps from fp32(score + ln g)")
    return dist


@pytest.mark.parametrize("spec", R.CASES, ids=R.case_id)
def test_sdpa_exact(ops, spec):
    B, N, T, H, dh, lens, seed, scale, sign = spec
    c, _, exp = R.case(spec)
    D, fails = H * dh, []
    bias = None if c["key_bias"] is None else c["key_bias"].to(DEV)
    kvl = None if c["kv_len"] is None else c["kv_len"].to(DEV)
    (_, q), (_, dout) = _window("q", B * N, D, c["q"]), _window("dout", B * N, D, c["dout"])
    want_out_f = _whole("out_fwd", B * N, D, exp["out"])
    want_out_d = _whole("out_fwd", B * N, D, exp["out_dense"])
    want_dq = _whole("dq", B * N, D, exp["dq"])
    delta_want = exp["delta"].to(DEV)
    worst = 0.0

    def run(tag, k_rows, k_data, v_data, vd_data, kv_off, want_dk, want_dv, works, kvl=kvl):
        nonlocal worst
        (_, k), (_, v) = _window("k", k_rows, D, k_data), _window("v", k_rows, D, vd_data)
        obuf, out = _window("out_fwd", B * N, D)                  # forward only, dense v: every column of out nonzero
        lse = torch.full((B, H, N), float("nan"), device=DEV)
        ops.sdpa_fwd(q, k, v, B, N, T, H, dh, scale, bias, kvl, out, lse, kv_off=kv_off)
        _check(fails, f"{tag} out (dense v)", obuf, want_out_d)
        worst = max(worst, _check_lse(fails, f"{tag} (dense v)", lse, exp))
        _, v = _window("v", k_rows, D, v_data)
        obuf, out = _window("out_fwd", B * N, D)
        lse = torch.full((B, H, N), float("nan"), device=DEV)
        ops.sdpa_fwd(q, k, v, B, N, T, H, dh, scale, bias, kvl, out, lse, kv_off=kv_off)
        _check(fails, f"{tag} out", obuf, want_out_f)
        worst = max(worst, _check_lse(fails, tag, lse, exp))
        _, out_b = _window("out_bwd", B * N, D, out)              # the backward reads 16-byte rows: ldo a multiple of 8
        for work in works:
            name = f"{tag} {'work list' if work is not None else 'dense'}"
            (qbuf, dq), (kbuf, dk), (vbuf, dv) = _window("dq", B * N, D), _window("dk", k_rows, D), _window("dv", k_rows, D)
            delta = torch.full((B, H, N), float("nan"), device=DEV)
            ops.sdpa_bwd(q, k, v, B, N, T, H, dh, scale, bias, kvl, out_b, dout, lse, delta, dq, dk, dv, work=work, parts=3,
                         kv_off=kv_off)
            if not torch.equal(delta, delta_want):
                fails.append(f"{name} delta: {(delta != delta_want).sum().item()} rows differ")
            _check(fails, f"{name} dq", qbuf, want_dq)
            _check(fails, f"{name} dk", kbuf, want_dk)
            _check(fails, f"{name} dv", vbuf, want_dv)

    works = [None] if lens is None else [None, ops.kv_work_list(list(lens), T, DEV)]
    run("padded", B * T, c["k"], c["v"], c["v_dense"], None, _whole("dk", B * T, D, exp["dk"]), _whole("dv", B * T, D, exp["dv"]), works)
    if lens is not None:
        # packed keys: the images' live rows back to back, then three rows of no image (guards in K / V, canaries in dK / dV)
        idx, off, rows = R.packed(c)
        tail = torch.full((3, D), GUARD, dtype=BF)
        kp, vp, vdp = (torch.cat([c[n][idx], tail]) for n in ("k", "v", "v_dense"))
        keep = torch.arange(rows)
        live = torch.tensor(c["live"], dtype=torch.int32, device=DEV)        # packed keys: kv_len >= 1, so T where it was 0
        run("packed", rows + 3, kp, vp, vdp, torch.tensor(off, dtype=torch.int32, device=DEV),
            _whole("dk", rows + 3, D, exp["dk"][idx], keep), _whole("dv", rows + 3, D, exp["dv"][idx], keep), works, kvl=live)
    torch.cuda.synchronize()
    print(f"[exact] {R.case_id(spec)}: lse at most {worst:.2f} fp32 ulps from the fp64 reference")
    assert not fails, "; ".join(fails)
