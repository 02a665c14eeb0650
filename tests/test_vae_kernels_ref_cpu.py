"""What test_vae_kernels_exact_gpu.py relies on, proved on the CPU (tests/vae_kernels_ref.py; no GPU, no yat_amd):

reach     every dispatch class the conv, GroupNorm and MSLA kernels have is reached by a named case (the maps are printed);
exact     every conv / MSLA sum is an integer that int64 arithmetic reproduces and whose partial sums fp32 holds in any
          order; every value at a rounding point is a bf16 number (round trip of the fp64 reference), except in the
          rounding-chain cases, where leaving out (or adding) any one rounding must move stored bits; SiLU sees saturated
          integers only; the GroupNorm populations have exact means, variance 4 a^2 and sums of squares below 2^24 steps;
bite      plain numpy executors that walk chunks, slabs and taps as the kernels do pass the checker on every case, and
          each planted error of vae_kernels_ref.FAULTS is caught by it on its targeted case.
"""
import numpy as np
import pytest
import torch

from tests import vae_kernels_ref as R

SAT = lambda v: bool((((v >= 32) & (v <= 255)) | ((v >= -255) & (v <= -128))).all())      # noqa: E731


def _is_bf16(v):
    return torch.equal(R.rb64(v), v)


def _show(title, m, capsys):
    with capsys.disabled():
        print(f"\n[{title}] class -> cases")
        for k in sorted(m):
            print(f"  {k:34s} {' '.join(m[k])}")


@pytest.fixture(scope="module")
def conv_built():
    out = {}
    for c in R.CONV_CASES:
        inp = R.conv_inputs(c)
        out[c["name"]] = (inp, *R.conv_expect(c, inp))
    return out


# ------------------------------------------------------------------------------------------------ reach
def test_conv_table_reaches_every_class(capsys):
    m = R.reached(R.CONV_CASES, R.conv_classes)
    _show("conv", m, capsys)
    missing = sorted(R.conv_required() - set(m))
    assert not missing, f"no case reaches {missing}"


def test_gn_table_reaches_every_class(capsys):
    m = R.reached(R.GN_CASES, R.gn_classes)
    _show("groupnorm", m, capsys)
    assert not sorted(R.GN_REQUIRED - set(m)), sorted(R.GN_REQUIRED - set(m))
    big = [c for c in R.GN_CASES if c["B"] * c["HW"] * c["C"] > 1 << 19]
    assert [c["name"] for c in big] == ["hw131073-c8"]                       # the one large case, about 1 M elements


def test_msla_table_reaches_every_class(capsys):
    m = R.reached(R.MSLA_CASES, R.msla_classes)
    _show("msla", m, capsys)
    assert not sorted(R.MSLA_REQUIRED - set(m)), sorted(R.MSLA_REQUIRED - set(m))


def test_conv_classes_restate_the_launch():
    """spot checks of the class function against hand-computed launches"""
    k = R.conv_classes(R.CONV_BY_NAME["dec-wg8"])
    assert {"dec/wg:=8", "dec/M:straddle", "dec/Cout:132", "dec/Cin:72"} <= k            # 405 pixels: 4 x 2 tiles
    assert {"down/wg:8q+7", "down/M:128k+1", "down/tapu:2"} <= R.conv_classes(R.CONV_BY_NAME["down-wg15"])
    assert "kl/grid:2x2in" in R.conv_classes(R.CONV_BY_NAME["kl-one"])
    assert "direct/stage:2" in R.conv_classes(R.CONV_BY_NAME["direct-c3"])


# ------------------------------------------------------------------------------------------------ exact: conv
@pytest.mark.parametrize("name", [c["name"] for c in R.CONV_CASES])
def test_conv_sums_and_rounding_points_are_exact(name, conv_built):
    c = R.CONV_BY_NAME[name]
    inp, want, stages = conv_built[name]
    S, P, H, W, g = R.conv_dims(c)
    # the weights: one +-1 in every 8-channel chunk of every tap of every output channel
    w8 = np.abs(inp["w"]).reshape(c["Cout"], 9, c["Cin"] // 8, 8)
    if c["thirds"]:
        assert not inp["w"].any() and inp["x"].reshape(-1, 3).sum(1).max() < 1 << 24
        assert torch.equal(R.ints_bf(inp["x"]).double(), torch.from_numpy(inp["x"]).double())
    else:
        assert (w8.sum(-1) == 1).all() and set(np.unique(inp["w"])) == {-1, 0, 1}
    if not (c["chain"] and c["kind"] != "dec") and not c["thirds"]:
        assert set(np.unique(inp["x"])) <= {-1, 0, 1} and (inp["x"] != 0).mean() > 0.4
    # integer sums: int64 chunk sums == the fp64 conv2d; every partial sum in any order is below 2^24
    acc, bound = R.conv_int_sums(c, inp)
    conv = stages["conv"].permute(0, 2, 3, 1).reshape(acc.shape)
    assert torch.equal(conv, torch.from_numpy(acc).double())
    assert bound < 1 << 24
    print(f"[conv] {name}: largest |sum| {np.abs(acc).max()}, largest sum of |products| {bound}")
    if "silu" in stages:                                  # the real function: x (1 - 1e-14) or -1e-54, bf16 makes it x or -0
        pre = R.rb64(stages["bias"])
        assert torch.equal(R.rb64(stages.pop("silu")), torch.where(pre > 0, pre, torch.zeros(()).double()))
    for st, v in stages.items():
        assert (st == "mean" and g == 3) or torch.equal(v.float().double(), v), f"{st}: fp32 does not hold the value"
    if not c["chain"]:
        for st, v in stages.items():
            if st in ("mean", "sum") and g == 3:
                continue                                  # thirds: numpy's float32 quotient (below); c + bf16(s) is exact in fp32
            assert _is_bf16(v), f"{st}: not a bf16 number before its rounding"
            if st not in ("mean", "sum"):
                assert v.abs().max() <= 256 and torch.equal(v, v.round())
    if g == 3:
        x = inp["x"]
        u = (x.reshape(c["B"], H // 2, 2, W // 2, 2, c["Cin"]).transpose(0, 1, 3, 5, 2, 4).reshape(c["B"], H // 2, W // 2, -1)
             if S == 2 else x)
        q = (u.reshape(*u.shape[:3], -1, 3).sum(-1).astype(np.float32) / np.float32(3)).astype(np.float32)
        s = torch.from_numpy(R._rbf_np(q).astype(np.float64)).permute(0, 3, 1, 2)
        assert torch.equal(s, R.rb64(stages["mean"]))


@pytest.mark.parametrize("name", [c["name"] for c in R.CONV_CASES if c["chain"]])
def test_chain_cases_notice_every_rounding(name, conv_built):
    """leaving out any rounding but the last, or rounding the conv sum before the bias, changes stored bits"""
    c = R.CONV_BY_NAME[name]
    inp, want, _ = conv_built[name]
    bits = R.to_bits(want)
    # SiLU is x on these values and rounds again: with it the rounding after the bias cannot show (dec-chain-sc1 has none)
    used = [r for r in R.ROUNDINGS[c["kind"]][:-1] if r != "silu" and (r != "sc" or c["sc_mode"]) and not (r == "bias" and c["silu"])]
    for r in used:
        other = R.to_bits(R.conv_expect(c, inp, skip=r)[0])
        n = int((R.fold(other) != R.fold(bits)).sum())
        print(f"[chain] {name}: without the rounding after {r}: {n} of {bits.numel()} elements change")
        assert n > 0, r
    if c["kind"] != "dec":
        n = int((R.fold(R.to_bits(R.conv_expect(c, inp, extra="conv")[0])) != R.fold(bits)).sum())
        print(f"[chain] {name}: with the conv sum rounded before the bias: {n} elements change")
        assert n > 0


def test_silu_preactivations_are_saturated(conv_built):
    for c in R.CONV_CASES:
        if c["silu"] and not c["chain"]:
            pre = R.rb64(conv_built[c["name"]][2]["bias"])
            assert SAT(pre), c["name"]
            assert np.array_equal(R.silu_f32(pre.numpy().astype(np.float32)), np.where(pre.numpy() > 0, pre.numpy(), -0.0))


# ------------------------------------------------------------------------------------------------ exact: groupnorm, msla
@pytest.mark.parametrize("name", sorted(R.GN_BY_NAME))
def test_gn_population_is_exact(name):
    c = R.GN_BY_NAME[name]
    inp = R.gn_inputs(c)
    B, HW, C, G, a = c["B"], c["HW"], c["C"], c["G"], c["a"]
    cg = C // G
    x = inp["x"].reshape(B, HW, G, cg)
    assert torch.equal(R.ints_bf(inp["x"]).double(), torch.from_numpy(inp["x"]).double())
    n = HW * cg
    assert (x.sum(axis=(1, 3)) == n * inp["mean"]).all()                                       # exact mean, int64
    d = x - inp["mean"][:, None, :, None]
    assert ((d * d).sum(axis=(1, 3)) == 4 * a * a * n).all()                                   # variance 4 a^2: rstd = 1 / (2a)
    assert (x[:, 0, :, 0] == inp["K"]).all() and (x >= inp["K"][:, None, :, None]).all()       # K first and least
    assert len({tuple(r) for r in inp["K"]}) == B or B == 1                                    # images differ
    # shifted sums: multiples of the step a, totals below 2^24 steps: exact in fp32 in any order
    sh = x - inp["K"][:, None, :, None]
    assert (sh % a == 0).all()
    t2 = ((sh // a) ** 2).sum(axis=(1, 3))
    print(f"[gn] {name}: largest total of squares {t2.max()} steps (2^24 = {1 << 24})")
    assert t2.max() < 1 << 24
    if HW > R.GN_SLAB:                                                                         # slab partials differ
        s0 = sh[:, :R.GN_SLAB].sum(axis=(1, 3))
        s1 = sh[:, R.GN_SLAB:2 * R.GN_SLAB].sum(axis=(1, 3))
        assert (s0 > 0).all() and (s0 != s1).any()
    want, pre = R.gn_expect(c, inp)
    closed = (d.reshape(B, HW, C) * inp["w"]) / (2.0 * a) + inp["b"]                           # xhat w + b, exact in fp64
    assert ((2 * closed) % 1 == 0).all() and np.abs(closed).max() <= 255
    assert torch.equal(pre, R.rb64(torch.from_numpy(closed)))
    ties = float((pre != torch.from_numpy(closed)).double().mean())
    print(f"[gn] {name}: {ties:.3f} of the outputs are ties between two bf16 numbers")
    assert ties > 0.9 if c["tie"] else ties == 0
    if c["silu"]:
        assert SAT(pre)
        assert torch.equal(want, torch.where(pre > 0, pre, torch.zeros(()).double()))
    assert R.mismatches(name, _buf(R.gn_exec(c, inp)), R.want_buffer(R.to_bits(want))) == []


@pytest.mark.parametrize("name", [c["name"] for c in R.MSLA_CASES])
def test_msla_sums_are_exact(name):
    c = next(k for k in R.MSLA_CASES if k["name"] == name)
    inp = R.msla_inputs(c)
    want, t = R.msla_expect(c, inp)
    assert set(np.unique(inp["wdw"])) == {-1, 0, 1} and (np.abs(inp["wpw"]).sum(1) == 4).all()
    assert len({tuple(r) for r in inp["wdw"]}) == c["C3"]                    # distinct per channel
    assert torch.equal(t, t.round()) and t.abs().max() <= 50 and _is_bf16(t)
    assert torch.equal(want, want.round()) and want.abs().max() <= 200
    assert R.mismatches(name, _buf(R.msla_exec(c, inp)), R.want_buffer(R.to_bits(want))) == []


def test_msla_tap_expectation_is_the_depthwise_conv():
    c = R.MSLA_TAP_CASE
    for tap in (0, 7, 12, 24):
        inp = R.msla_tap_inputs(c, tap)
        want = torch.from_numpy(R.msla_tap_expect(c, inp, tap)).double()
        assert torch.equal(R.msla_expect(c, inp)[0], want)
        assert R.mismatches(f"tap {tap}", _buf(R.msla_exec(c, inp)), R.want_buffer(R.to_bits(want))) == []


# ------------------------------------------------------------------------------------------------ bite
def _buf(bits):
    """the executor's output inside a canary buffer, as the GPU file reads one back"""
    b = R.out_buffer(bits.numel())
    b[R.LEAD:R.LEAD + bits.numel()] = bits.reshape(-1)
    return b


def test_checker_names_the_first_bad_index():
    w = R.want_buffer(R.to_bits(torch.tensor([1.0, -0.0, 3.0]).double()))
    g = w.clone()
    assert R.mismatches("x", g, w) == []
    g[R.LEAD + 1] = -32768                                                    # -0 where +0 is expected: equal
    assert R.mismatches("x", g, w) == []
    g[R.LEAD + 2] = 0x4000
    assert "element 2: bits 0x4000, expected 0x4040" in R.mismatches("x", g, w)[0]
    g = w.clone()
    g[-1] = 0
    assert "behind the output" in R.mismatches("x", g, w)[0]
    g = w.clone()
    g[0] = 0
    assert "before the output" in R.mismatches("x", g, w)[0]


def test_correct_conv_executor_passes_every_case(conv_built):
    fails = []
    for c in R.CONV_CASES:
        inp, want, _ = conv_built[c["name"]]
        fails += R.mismatches(c["name"], _buf(R.conv_exec(c, inp)), R.want_buffer(R.to_bits(want)))
    assert not fails, "; ".join(fails[:6])


CONV_FAULT_TARGETS = [("drop_chunk", "dec-k1024"), ("drop_chunk", "kl-wg15"), ("tail_quad", "mean-wg8"), ("tail_quad", "dec-m128"),
                      ("sc_index", "dec-wg11"), ("sc_index", "dec-up-sc2r1"), ("skip_round", "dec-chain-sc1"),
                      ("skip_round", "down-chain"), ("skip_round", "mean-chain"), ("inv_quotient", "mean-thirds")]


@pytest.mark.parametrize("fault,name", CONV_FAULT_TARGETS)
def test_planted_conv_error_is_caught(fault, name, conv_built):
    c = R.CONV_BY_NAME[name]
    inp, want, _ = conv_built[name]
    got = R.mismatches(name, _buf(R.conv_exec(c, inp, fault)), R.want_buffer(R.to_bits(want)))
    print(got)
    assert got and "elements differ, first at element" in got[0]


@pytest.mark.parametrize("fault,name", [("drop_slab", "hw513-c128"), ("drop_slab", "hw131073-c8"), ("drop_slab", "hw512-c24"), ("neighbour_stat", "hw511-c96"),
                                        ("neighbour_stat", "hw1-c128")])
def test_planted_gn_error_is_caught(fault, name):
    c = R.GN_BY_NAME[name]
    inp = R.gn_inputs(c)
    got = R.mismatches(name, _buf(R.gn_exec(c, inp, fault)), R.want_buffer(R.to_bits(R.gn_expect(c, inp)[0])))
    print(got)
    assert got


def test_planted_msla_error_is_caught():
    for c in R.MSLA_CASES:
        inp = R.msla_inputs(c)
        assert R.mismatches(c["name"], _buf(R.msla_exec(c, inp, "missing_tap")), R.want_buffer(R.to_bits(R.msla_expect(c, inp)[0])))
    c = R.MSLA_TAP_CASE
    inp = R.msla_tap_inputs(c, 12)
    want = torch.from_numpy(R.msla_tap_expect(c, inp, 12)).double()
    assert R.mismatches("tap 12", _buf(R.msla_exec(c, inp, "missing_tap")), R.want_buffer(R.to_bits(want)))


def test_small_sums_cannot_tell_the_quotient_from_the_product(conv_built):
    """on sums of {-1, 0, 1} the planted a * (1 / 3) gives the bits of a / 3: why mean-thirds exists"""
    for name in ("mean-g3", "down-g3"):
        c = R.CONV_BY_NAME[name]
        inp, want, _ = conv_built[name]
        assert R.mismatches(name, _buf(R.conv_exec(c, inp, "inv_quotient")), R.want_buffer(R.to_bits(want))) == []
    x = conv_built["mean-thirds"][0]["x"]
    assert len(R.thirds_triples()) >= 8 and len({tuple(t) for t in x.reshape(-1, 3)}) >= 40


def test_every_fault_has_a_target():
    named = {f for f, _ in CONV_FAULT_TARGETS} | {"drop_slab", "neighbour_stat", "missing_tap"}
    assert named == set(R.FAULTS)
