"""The VAE kernels held to exact results -- GPU: the shared 3x3 implicit-GEMM conv through its four entry points
(yat_dcae_conv3x3, yat_dcae_conv3x3_mean, yat_dcae_conv3x3_down, yat_vae_conv3x3_down) and the direct kernel for Cout <= 4,
yat_vae_groupnorm (eps = 0) and yat_dcae_msla_aggregate.

Inputs, plain fp64 references and the case lists come from tests/vae_kernels_ref.py; test_vae_kernels_ref_cpu.py proves that
the lists reach every dispatch class, that every sum is exact in fp32 in any order and that the expected bits need no device
arithmetic.  Nothing is compared with another run of a kernel.  Every output sits behind 16 and before 24 canary elements
(bf16 bits 0x7FC1) and the buffer is compared whole, on bits, -0 folded onto +0; every input is read back after the launch and
must be unchanged; the GroupNorm workspace starts as a canary and keeps its tail.  Each test collects all its mismatches
before it fails and names the first bad index with both bit patterns.
"""
import numpy as np
import pytest
import torch

from tests import vae_kernels_ref as R
from tests.gpu_common import BF, DEV

pytestmark = pytest.mark.gpu
I16 = torch.int16


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


# ------------------------------------------------------------------------------------------------ buffers
def out_view(n):
    """(whole canary buffer on the device, bf16 view of the n elements a kernel is to write)"""
    buf = R.out_buffer(n).to(DEV)
    return buf, buf.view(BF)[R.LEAD:R.LEAD + n]


class Inputs:
    """device copies of integer operands, with the bits they must still hold after the launch"""

    def __init__(self):
        self.kept = []

    def __call__(self, name, a):
        if a is None:
            return None
        t = R.ints_bf(a)
        d = t.to(DEV)
        self.kept.append((name, d, R.bf_bits(t)))
        return d

    def unchanged(self, fails, what):
        for name, d, bits in self.kept:
            if not torch.equal(d.view(I16).cpu(), bits):
                fails.append(f"{what}: the launch changed its input {name}")


def check(fails, what, buf, want):
    torch.cuda.synchronize()
    fails += R.mismatches(what, buf.cpu(), R.want_buffer(R.to_bits(want)))


# ------------------------------------------------------------------------------------------------ conv
@pytest.fixture(scope="module")
def conv_ref():
    """case name -> (inputs, expected values): computed once, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            c = R.CONV_BY_NAME[name]
            inp = R.conv_inputs(c)
            cache[name] = (inp, R.conv_expect(c, inp)[0])
        return cache[name]
    return get


def run_conv(ops, c, d, y):
    B, Cin, Cout = c["B"], c["Cin"], c["Cout"]
    S, P, H, W, g = R.conv_dims(c)
    if c["kind"] in ("dec", "direct"):
        sc = d["x"] if c["sc_mode"] and not c["sc_own"] else d["sc"]
        ops.dcae_conv3x3(d["x"], d["w"], y, B, c["Ho"], c["Wo"], Cin, Cout, bias=d["bias"], upsample=bool(c["up"]),
                         silu=bool(c["silu"]), shortcut_mode=c["sc_mode"], shortcut=sc, shortcut_channels=R.conv_sc_channels(c),
                         residual=d["res"], out_nchw=bool(c["nchw"]))
    elif c["kind"] == "mean":
        ops.dcae_conv3x3_mean(d["x"], d["w"], y, B, H, W, Cin, Cout, bias=d["bias"], shortcut=bool(c["shortcut"]))
    elif c["kind"] == "down":
        ops.dcae_conv3x3_down(d["x"], d["w"], y, B, H, W, Cin, Cout, bias=d["bias"], shortcut=bool(c["shortcut"]))
    else:
        ops.vae_conv3x3_down(d["x"], d["w"], y, B, H, W, Cin, Cout, bias=d["bias"])


@pytest.mark.parametrize("name", [c["name"] for c in R.CONV_CASES])
def test_conv3x3(ops, conv_ref, name):
    c = R.CONV_BY_NAME[name]
    inp, want = conv_ref(name)
    put = Inputs()
    d = {k: put(k, inp[k]) for k in ("x", "w", "bias", "res")}
    d["sc"] = put("sc", inp["sc"]) if c["sc_own"] else None
    buf, y = out_view(want.numel())
    run_conv(ops, c, d, y.view(want.shape))
    fails = []
    check(fails, name, buf, want)
    put.unchanged(fails, name)
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ groupnorm
def gn_workspace(ops, c):
    n = ops.vae_groupnorm_workspace_bytes(c["B"], c["HW"], c["C"], c["G"]) // 4
    assert n == R.gn_workspace_floats(c["B"], c["HW"], c["G"])
    return torch.full((n + 8,), R.WS_CANARY, dtype=torch.int32, device=DEV), n


def run_gn(ops, fails, c, ws, n, what):
    """one call on the workspace ``ws``: separate output or in place, as the case says"""
    inp = R.gn_inputs(c)
    want = R.gn_expect(c, inp)[0]
    put = Inputs()
    w, b = put("w", inp["w"]), put("b", inp["b"])
    buf, y = out_view(want.numel())
    y = y.view(c["B"], c["HW"], c["C"])
    if c["inplace"]:
        y.copy_(R.ints_bf(inp["x"]))
        x = y
    else:
        x = put("x", inp["x"])
    ops.vae_groupnorm(x, w, b, y, c["B"], c["HW"], c["C"], c["G"], ws[:n], eps=0.0, silu=bool(c["silu"]))
    check(fails, what, buf, want)
    put.unchanged(fails, what)
    if not bool((ws[n:] == R.WS_CANARY).all()):
        fails.append(f"{what}: wrote behind the workspace")
    st = ws[:n].view(torch.float32)[n - c["B"] * c["G"] * 4:].view(c["B"], c["G"], 4).cpu().double().numpy()
    for k, (name, exact) in enumerate((("K", inp["K"]), ("mean - K", inp["mean"] - inp["K"]), ("rstd", 0.5 / c["a"] + 0 * inp["K"]))):
        if not np.array_equal(st[..., k], exact):
            fails.append(f"{what}: the statistic {name} of {int((st[..., k] != exact).sum())} groups is not the exact value")


@pytest.mark.parametrize("name", [c["name"] for c in R.GN_CASES])
def test_groupnorm(ops, name):
    c = R.GN_BY_NAME[name]
    ws, n = gn_workspace(ops, c)
    fails = []
    run_gn(ops, fails, c, ws, n, name)
    assert not fails, "; ".join(fails)


def test_groupnorm_second_call_on_the_same_workspace(ops):
    """other data, other statistics: nothing of the first call may survive in the partials or the statistics"""
    first, second = R.GN_BY_NAME["hw64-c24"], R.GN_SECOND
    ws, n = gn_workspace(ops, first)
    fails = []
    for c in (first, second, first):
        run_gn(ops, fails, c, ws, n, c["name"])
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ msla_aggregate
def run_msla(ops, fails, c, inp, want, what):
    put = Inputs()
    x, wdw, wpw = put("x", inp["x"]), put("w_dw", inp["wdw"]), put("w_pw", inp["wpw"])
    buf, y = out_view(want.numel())
    ops.dcae_msla_aggregate(x, wdw, wpw, y.view(want.shape), c["B"], c["H"], c["W"], c["C3"])
    check(fails, what, buf, want)
    put.unchanged(fails, what)


@pytest.mark.parametrize("name", [c["name"] for c in R.MSLA_CASES])
def test_msla_aggregate(ops, name):
    c = next(k for k in R.MSLA_CASES if k["name"] == name)
    inp = R.msla_inputs(c)
    fails = []
    run_msla(ops, fails, c, inp, R.msla_expect(c, inp)[0], name)
    assert not fails, "; ".join(fails)


def test_msla_tap_placement_is_exact(ops):
    """one depthwise tap of weight 1 at a time, identity pointwise map: the output is the input pixel that tap reads,
    (y + ty - 2, x + tx - 2), bit for bit, and exact zeros where that lies outside the image"""
    c = R.MSLA_TAP_CASE
    fails = []
    for tap in range(25):
        inp = R.msla_tap_inputs(c, tap)
        run_msla(ops, fails, c, inp, torch.from_numpy(R.msla_tap_expect(c, inp, tap)).double(), f"tap ({tap // 5}, {tap % 5})")
    assert not fails, "; ".join(fails[:6])
