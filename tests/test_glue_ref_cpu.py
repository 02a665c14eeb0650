"""What tests/test_glue_exact_gpu.py relies on, proven on the CPU: every launch class of the case lists in tests/glue_ref.py
is reached, the integer sums stay exact, the saturated-input identities hold in the fp32 model of the library's formulas,
the round-to-nearest-even table agrees with torch, and the splitmix64 reference agrees with pure-Python integers.  Also the
argument checks of the yat_amd.ops wrappers that hand the library an element count and raw pointers: they raise ValueError
before any library call, so no GPU is needed."""
import numpy as np
import pytest
import torch

from tests import glue_ref as R

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ launch classes
def test_ew_cases_reach_every_class():
    c = {n: R.ew_classes(n) for n in R.EW_N}
    assert [n for n in R.EW_N if c[n]["vectors"] == 0 and c[n]["tail"]] == [1, 7]               # scalar tail alone
    assert c[8]["vectors"] == 1 and c[8]["tail"] == 0 and c[9]["tail"] == 1
    assert c[2048 * 8 + 3]["blocks"] == 8 and c[2048 * 8 + 3]["passes"] == 1 and c[2048 * 8 + 3]["tail"] == 3
    full = c[4194304]
    assert full["blocks"] == R.EW_CAP and full["passes"] == 1 and not full["ragged"] and not full["capped"]
    one = c[4194304 + 8]                                           # one vector in the second pass
    assert one["capped"] and one["passes"] == 2 and one["vectors"] - R.EW_CAP * 256 == 1
    two = c[4194304 + 8 * 257 + 5]                                 # second pass spills into a second workgroup, with a tail
    assert two["passes"] == 2 and two["vectors"] - R.EW_CAP * 256 == 257 and two["tail"] == 5
    last = c[3 * 4194304 + 13]
    assert last["passes"] == 4 and last["tail"] == 5


def test_stride_cases_reach_the_wrap():
    cap = R.EW_CAP * 256                                           # flow_mix, dropout, f32_to_bf16: 524,288 elements
    assert cap == 524288
    for lst in ([B * per for B, per in R.FLOW_CASES], R.DROP_N, R.F32_N + [len(R.rne_table()[0])]):
        passes = [R.stride_classes(n, R.EW_CAP)["passes"] for n in lst]
        assert 1 in passes and 2 in passes and any(n == cap + 1 for n in lst), lst
    assert 524288 in R.DROP_N and 524288 in R.F32_N                # exactly one full pass
    assert R.stride_classes(R.DROP_N[-1], R.EW_CAP)["passes"] == 4
    B, per = R.FLOW_CASES[-1]
    assert per % 256 and per % 8 and (2 * per) % 256               # sample borders aligned to nothing
    pix = R.PIX_CAP * 256
    assert pix == 1048576
    assert [R.stride_classes(B * per, R.PIX_CAP)["passes"] for B, per in R.DDPM_CASES] == [1, 1, 2]
    assert [R.stride_classes(B * C * H * W, R.PIX_CAP)["passes"] for B, C, H, W, p in R.PATCH_CASES][-1] == 2
    assert 4 * 514 * 514 > pix
    assert {(p, C) for _, C, _, _, p in R.PATCH_CASES[:-1]} == {(p, C) for p in (1, 2, 4) for C in (1, 3, 4)}
    assert all(H != W for _, _, H, W, _ in R.PATCH_CASES[:-1])
    rows, N, D = R.POS_CASES[-1]
    assert rows % N == 0 and rows * (D // 8) == 1048608 and R.stride_classes(rows * (D // 8), R.PIX_CAP)["passes"] == 2
    assert {(D, rows // N) for rows, N, D in R.POS_CASES[:-1]} == {(8, 1), (8, 3), (1152, 1), (1152, 3)}
    B, N, T, C = R.JOINT_CASES[-1]
    chunks = B * (N + T) * (C // 8)
    assert chunks > R.JOINT_CAP * 256 == 2097152 and R.stride_classes(chunks, R.JOINT_CAP)["passes"] == 2
    assert {(T, C) for _, _, T, C in R.JOINT_CASES[:-1]} == {(T, C) for T in (0, 1, 154) for C in (8, 1536)}
    assert B * (N + T) * C * 2 < 36e6                              # the largest case moves about 35 MB
    assert max(B * (N + T) for B, N, T, _, _ in R.QKNORM_CASES) > R.QKNORM_CAP
    assert {dh for *_, dh in R.QKNORM_CASES} == {32, 64, 128} and any(T == 0 for _, _, T, _, _ in R.QKNORM_CASES)
    assert [B * (d // 2) > 256 for B, d in R.TSTEP_CASES] == [False, True, False, True]
    assert any((d // 2) % 2 for _, d in R.TSTEP_CASES[1:])          # an odd half


def test_mse_cases_reach_every_class():
    c = {n: R.mse_classes(n) for n in R.MSE_N}
    assert c[1]["blocks"] == 1 and c[255]["blocks"] == 1 and c[256]["blocks"] == 1 and c[257]["blocks"] == 2
    assert c[65536]["blocks"] == 256 and c[65536]["passes"] == 1 and not c[65536]["ragged"]
    assert c[65537]["passes"] == 2 and c[3 * 65536 + 77]["passes"] == 4 and c[2 ** 18]["passes"] == 4
    assert {c[n]["final_passes"] for n in R.MSE_N} == {1, 4}        # mse_final_kernel: one pass and four of its 64 lanes
    assert max(R.MSE_N) == 2 ** 18
    assert [R.mse_classes(B * s)["passes"] for B, _, s in R.MSE_CHUNK] == [1, 1, 1, 2]
    assert R.mse_classes(4 * 16384)["blocks"] == 256 and not R.mse_classes(4 * 16384)["ragged"]
    assert [u < s for _, u, s in R.MSE_CHUNK] == [True, True, False, True]


def test_text_cases_reach_every_class():
    assert [R.text_classes(1, 1, C)["chunks"] for C in R.TEXT_C] == [1, 63, 64, 65, 129]
    assert [R.text_classes(1, 1, C)["chunk_passes"] for C in R.TEXT_C] == [1, 1, 1, 2, 3]
    assert [B * T % 4 for B, T, _ in R.TEXT_BT] == [1, 2, 3, 0]
    rel = set()
    for B, T, lens in R.TEXT_BT:
        assert len(lens) == B
        rel |= {0 if L == 0 else 1 if L == 1 else "T" if L == T else "T+3" if L == T + 3 else None for L in lens}
        for rp in R.pack_rows_padded(B, T, lens):
            assert rp >= sum(lens)
            rel.add(("<" if rp < B * T else "=" if rp == B * T else ">", "=" if rp == sum(lens) else "<"))
    assert {0, 1, "T", "T+3"} <= rel
    assert {(a, b) for a in "<=>" for b in "=<"} <= rel
    # a caption longer than T is not the last one somewhere: the next caption's rows must not leak into it
    assert any(L > T and b + 1 < B for B, T, lens in R.TEXT_BT for b, L in enumerate(lens))


# ------------------------------------------------------------------------------------------------ exact sums
def test_sums_stay_exact():
    for n in (1, 9, 4194304 + 8 * 257 + 5):
        a, b, want = R.add_case(n)
        s = a.double() + b.double()
        assert s.abs().max() <= 128 and torch.equal(s, s.to(BF).double())       # every sum is a bf16 number
        assert torch.equal(R.fold(R.bf_bits(s.to(BF))), want)
    for n in R.MSE_N:
        pred, target, d, S = R.mse_case(n)
        assert np.abs(d).max() <= 8 and n <= 2 ** 18 and S < 2 ** 24
        assert torch.equal(pred.double() - target.double(), torch.from_numpy(d).double())
        # any partial sum of the squares is an integer below 2^24: exact in fp32 in any order
        assert float(np.float32(S)) == S
    for B, used, stride in R.MSE_CHUNK:
        pred, target = R.chunk_case(B, used, stride, real=False)
        d = pred[:, :used].double() - target.double()
        assert d.abs().max() <= 4 and (d * d).sum() < 2 ** 24
        assert torch.equal(d, d.to(BF).double()) and torch.equal(d * d, (d * d).to(BF).double())
    for rows, N, D in R.POS_CASES[:-1]:
        x, pos, want, s = R.pos_case(rows, N, D)
        exact = x.double().view(rows // N, N, D) + pos.double()[None]
        assert np.array_equal(exact.view(rows, D).numpy(), s.astype(np.float64))   # the fp32 sum is exact
        frac_tie = ((np.abs(s) >= 128) & (np.abs(s) < 256)).mean()
        assert frac_tie > 0.5                                       # ... and mostly an exact tie between two bf16 numbers
        tie = torch.from_numpy((np.abs(s) >= 128) & (np.abs(s) < 256))
        assert (want.float()[tie] % 2 == 0).all()                   # rounded to even


def test_copy_pattern_carries_every_kind_of_bits():
    b = R.pattern(70000).numpy().view(np.uint16)
    assert b[65520] == 65520 and b[65521] == 0 and len(np.unique(b)) == R.MOD
    assert 0x7FC0 in b and 0x8000 in b and 0x0001 in b and 0xFF80 in b


# ------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("name", ["silu", "gelu_tanh", "dsilu", "dgelu_tanh"])
def test_saturated_identities_hold_in_the_fp32_model(name):
    x = np.concatenate([np.arange(32, 256), -np.arange(128, 256)]).astype(np.float32)
    assert set(R.saturated(352).tolist()) == set(x.tolist())
    y = R.model_f32(name, x)
    pos = x > 0
    want = x[pos] if not name.startswith("d") else np.ones(pos.sum(), np.float32)
    assert np.array_equal(y[pos], want)
    assert (y[~pos] == 0).all() and np.signbit(y[~pos]).all()       # exactly -0
    if name == "dgelu_tanh":
        assert np.array_equal(R.model_f32(name, x, clamp=False).view(np.uint32), y.view(np.uint32))


def test_ew_case_expectations():
    x, dy, fwd, bwd = R.ew_case(1000)
    assert torch.equal(fwd.view(BF).float(), torch.where(x.float() > 0, x.float(), torch.zeros(())))
    assert torch.equal(bwd.view(BF).float(), torch.where(x.float() > 0, dy.float(), torch.zeros(())))
    assert (dy.float().abs() <= 6).all() and (x.float() > 0).any() and (x.float() < 0).any()


def test_fp32_model_excess_over_the_reference():
    """Measured here, in bf16 ulps (dy = 1 / dy = -3): silu 0.0000, gelu_tanh 0.0001, dsilu 0.0018 / 0.0029 at x = -1.28,
    dgelu_tanh 0.0011 / 0.0017 at x = -0.75 -- the derivatives are worst where they cross zero.  The sweep's m is 8 x the
    largest: 0.023."""
    worst = {}
    for name, dy, *fused in R.ACT_MODELS:
        e, at = R.act_excess(name, dy, *fused)
        print(f"[model] {name} dy={dy:g}{' (not contracted)' if fused else ''}: fp32 model at most {e:.4f} bf16 ulps from the fp64 reference (x = {at:g})")
        worst[name] = max(worst.get(name, 0.0), e)
    assert max(worst["dgelu_tanh"], worst["dsilu"]) < 0.01 and max(worst["silu"], worst["gelu_tanh"]) < 0.0011
    assert R.act_margin() == 8.0 * max(worst.values()) and R.act_margin() < 0.08


def test_reference_agrees_with_torch_fp64():
    """the cancellation-free fp64 forms are the functions torch evaluates (compared where torch's own form keeps digits)"""
    x = np.linspace(-6.0, 6.0, 4801)
    t = torch.from_numpy(x).requires_grad_(True)
    for name, f in (("silu", torch.nn.functional.silu), ("gelu_tanh", lambda v: torch.nn.functional.gelu(v, approximate="tanh"))):
        y = f(t)
        g, = torch.autograd.grad(y.sum(), t)
        assert np.abs(R.ref_f64(name, x) - y.detach().numpy()).max() < 1e-14
        assert np.abs(R.ref_f64("d" + name, x) - g.numpy()).max() < 1e-13


def test_dgelu_band():
    """Without the clamp the fp32 formula gives NaN for x <= -1.17e13 (x (1 - s) u' overflows to -inf, times s = 0); torch's
    fp32 backward is finite (0) there down to about -5e19.  With the clamp the model is finite on every finite negative x,
    and every input outside the band keeps its bits."""
    _, x = R.all_bf16()
    fin = np.isfinite(x)
    old, new = R.model_f32("dgelu_tanh", x, clamp=False), R.model_f32("dgelu_tanh", x)
    band = fin & np.isnan(old) & (x < 0)
    assert band.any() and -1.18e13 < x[band].max() < -1.16e13
    assert np.array_equal(band, fin & (x <= x[band].max()))        # every finite input from there down
    assert (new[band] == 0).all()
    same = ~band & (x != -np.inf)                                   # (-inf goes from NaN to -0 with the band)
    assert np.array_equal(old[same].view(np.uint32), new[same].view(np.uint32))
    tor = R.torch_f32("dgelu_tanh", x)
    lost = fin & np.isfinite(tor) & ~np.isfinite(new)
    assert not lost.any(), x[lost]
    assert np.isnan(new[np.isnan(x)]).all()                         # NaN still propagates
    tb = band & np.isfinite(tor)
    print(f"[model] dgelu band: NaN before the clamp on {band.sum()} inputs, x in [{x[band].min():g}, {x[band].max():g}]; torch "
          f"is finite on {tb.sum()} of them, down to x = {x[tb].min():g}")


# ------------------------------------------------------------------------------------------------ rounding
def test_rne_table_agrees_with_torch():
    u, r, nan = R.rne_table()
    assert len(u) == 65536 * 6
    got = torch.from_numpy(u.view(np.float32).copy()).to(BF).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got[~nan], r[~nan])
    assert torch.from_numpy(got[nan].view(np.int16).copy()).view(BF).isnan().all()
    f = u.view(np.float32)
    fin = ~nan & np.isfinite(f)
    out = (r.astype(np.uint32) << 16).view(np.float32)
    assert np.isinf(out[fin]).any()                                 # overflow to inf by rounding
    assert ((r[fin] & 0x7F) == 0)[(u[fin] & 0xFFFF) == 0xFFFF].any()    # a carry through the whole mantissa
    assert ((u & 0x7F800000) == 0).any() and (u & 0xFFFF == 0x8000).any()   # denormals and exact ties
    assert np.array_equal(R._rbf_np(f[fin]).view(np.uint32) >> 16, r[fin].astype(np.uint32))
    for n in R.F32_N:
        un, rn, nn = R.rne_case(n)
        assert len(un) == n


def test_splitmix64_agrees_with_python_integers():
    for seed in R.DROP_SEEDS:
        for start, n in ((0, 300), (524288 - 3, 6), (3 * 524288, 5), (2 ** 32 - 2, 4)):
            got = R.splitmix_np(seed, n, start)
            assert got.tolist() == [R.splitmix_py(seed, start + i) for i in range(n)]
            assert got.max() < 2 ** 24
    assert [R.drop_thresh(p) for p in R.DROP_P] == [0, 1, int(np.float32(0.3) * np.float32(2 ** 24)), 2 ** 24 - 1]
    # the mask does not repeat at the grid wrap
    m = R.splitmix_np(12345, 2 * 524288)
    assert not np.array_equal(m[:524288], m[524288:])
    keep = R.drop_keep(12345, 1 << 20, 0.3)
    assert abs(keep.float().mean().item() - 0.7) < 3e-3
    assert R.drop_keep(0, 1000, 0.0).all() and R.drop_keep(7, 100000, 1.0 - 2.0 ** -24).sum() <= 1


def test_layout_references():
    img = R.pattern(2 * 3 * 4 * 6).view(2, 3, 4, 6)
    unf = torch.nn.functional.unfold(img.double(), kernel_size=2, stride=2).transpose(1, 2).reshape(2 * 2 * 3, 3 * 4)
    assert torch.equal(R.patch_ref(img, 2, True).double(), unf)     # channel-major = the im2col rows of Conv2d(k=p, s=p)
    tok = R.patch_ref(img, 2, False)
    assert torch.equal(R.unpatchify_ref(tok, 2, 3, 4, 6, 2), img)
    assert torch.equal(R.unpatchify_ref(tok, 2, 3, 4, 6, 2).double(),
                       torch.einsum("nhwpqc->nchpwq", tok.double().reshape(2, 2, 3, 2, 2, 3)).reshape(2, 3, 4, 6))
    src, offs, dst, mask, bias, kvl = R.text_case(3, 5, 8, [1, 8, 5])
    assert kvl.tolist() == [1, 5, 5] and mask.view(3, 5).sum(1).tolist() == [1, 5, 5] and offs.tolist() == [0, 1, 9, 14]
    assert torch.equal(dst[5:10], src[1:6]) and torch.equal(dst[10:15], src[9:14]) and (dst[1:5] == 0).all()
    assert (bias.view(3, 5)[0, 1:] == -9984.0).all() and (src[14:] == R.GUARD).all()
    _, _, packed, *_ = R.text_case(3, 5, 8, [1, 8, 5], rows_padded=16)
    assert torch.equal(packed[:14], src[:14]) and (packed[14:] == 0).all()
    i, t, j = R.joint_case(2, 5, 1, 8)
    assert torch.equal(j[:5], i[:5]) and torch.equal(j[5], t[0]) and torch.equal(j[6:11], i[5:]) and torch.equal(j[11], t[1])


def test_qknorm_inputs_keep_off_the_ties():
    """the forward's expected bits do not depend on the order of the fp32 sum of squares: every normalised element is
    TIE_MARGIN from a tie, and the fp32 restatement gives the bits of the fp64 one"""
    for B, N, T, H, dh in R.QKNORM_CASES:
        D = H * dh
        for rows, seed in ((B * N, 1), (B * T, 2)):
            if not rows:
                continue
            t = R.qknorm_inputs(rows, D, seed, 5, dh)
            qk = t[:, :2 * D]
            assert R.tie_distance(qk, dh).min() >= R.TIE_MARGIN
            plain = R.qknorm_inputs(rows, D, seed, 5)
            moved = (qk != plain[:, :2 * D]).sum().item()
            assert moved <= max(2, 0.02 * qk.numel()) and torch.equal(R.bf_bits(t[:, 2 * D:]), R.bf_bits(plain[:, 2 * D:]))
            x = qk.reshape(-1, dh)
            y32 = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + R.QKNORM_EPS)).to(BF)
            y64 = (x.double() * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + R.QKNORM_EPS)).to(BF)
            assert torch.equal(y32, y64)
            # an fp32 evaluation is off by a few 2^-24: an order of magnitude inside the margin
            r32 = torch.rsqrt(x.float().pow(2).mean(-1) + R.QKNORM_EPS).double()
            r64 = torch.rsqrt(x.double().pow(2).mean(-1) + R.QKNORM_EPS)
            assert ((r32 - r64).abs() / r64).max() < 2.0 ** -21 < R.TIE_MARGIN * 2.0 ** -8 / 8


# ------------------------------------------------------------------------------------------------ wrapper argument checks
@pytest.fixture
def ops(monkeypatch):
    """yat_amd.ops with the library replaced by a tripwire: a check that passes reaches it, a check that raises does not"""
    from yat_amd import ops as o

    class Reached(Exception):
        pass

    def lib():
        raise Reached
    monkeypatch.setattr(o, "_lib", lib)
    monkeypatch.setattr(o, "Reached", Reached, raising=False)
    return o


def _bf(*shape):
    return torch.zeros(*shape, dtype=BF)


def _calls(o):
    """name -> (callable on a dict of arguments, good arguments, [(argument, bad value, why)])"""
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    strided = _bf(8, 8)[:, :4]
    text = dict(src=_bf(7, 16), offs=torch.zeros(4, dtype=i32), dst=_bf(3 * 5, 16), mask=torch.zeros(15, dtype=i64),
                bias=torch.zeros(15), kvl=torch.zeros(3, dtype=i32))
    text_bad = [("src", _bf(7, 16).float(), "dtype"), ("src", _bf(7, 32)[:, :16], "strided"), ("dst", _bf(15, 16).half(), "dtype"),
                ("dst", _bf(15, 32)[:, :16], "strided"), ("offs", torch.zeros(4, dtype=i64), "dtype"),
                ("offs", torch.zeros(3, dtype=i32), "count"), ("mask", torch.zeros(15, dtype=i32), "dtype"),
                ("mask", torch.zeros(14, dtype=i64), "count"), ("bias", torch.zeros(15, dtype=BF), "dtype"),
                ("bias", torch.zeros(15, 2)[:, 0], "strided"), ("kvl", torch.zeros(3, dtype=i64), "dtype"),
                ("kvl", torch.zeros(2, dtype=i32), "count")]
    return {
        "act_fwd": (lambda a: o.act_fwd(a["x"], "silu", a["y"]), dict(x=_bf(4, 8), y=_bf(4, 8)),
                    [("x", _bf(4, 8).float(), "dtype"), ("x", strided, "strided"), ("y", _bf(4, 7), "count"), ("y", _bf(32).half(), "dtype"),
                     ("y", _bf(8, 8)[:, :4], "strided")]),
        "act_bwd": (lambda a: o.act_bwd(a["x"], a["dy"], "gelu_tanh", a["dx"]), dict(x=_bf(4, 8), dy=_bf(4, 8), dx=_bf(4, 8)),
                    [("x", strided, "strided"), ("dy", _bf(3, 8), "count"), ("dy", _bf(4, 8).float(), "dtype"), ("dy", _bf(4, 16)[:, :8], "strided"),
                     ("dx", _bf(5, 8), "count"), ("dx", _bf(4, 8).float(), "dtype")]),
        "add_bf16": (lambda a: o.add_bf16(a["a"], a["b"], a["out"]), dict(a=_bf(6), b=_bf(6), out=_bf(6)),
                     [("a", _bf(6).float(), "dtype"), ("b", _bf(5), "count"), ("b", _bf(12)[::2], "strided"), ("out", _bf(7), "count"),
                      ("out", _bf(6).float(), "dtype")]),
        "f32_to_bf16": (lambda a: o.f32_to_bf16(a["x"], a["y"]), dict(x=torch.zeros(9), y=_bf(9)),
                        [("x", _bf(9), "dtype"), ("x", torch.zeros(18)[::2], "strided"), ("y", torch.zeros(9), "dtype"), ("y", _bf(8), "count"),
                         ("y", _bf(18)[::2], "strided")]),
        "transpose": (lambda a: o.transpose(a["x"], a["out"]), dict(x=_bf(2, 3, 4), out=_bf(2, 4, 3)),
                      [("x", _bf(2, 3, 4).float(), "dtype"), ("x", _bf(2, 3, 8)[:, :, :4], "strided"), ("x", _bf(6, 4), "rank"),
                       ("out", _bf(2, 4, 2), "count"), ("out", _bf(2, 4, 3).float(), "dtype"), ("out", _bf(2, 4, 6)[:, :, :3], "strided")]),
        "timestep_embed": (lambda a: o.timestep_embed(a["t"], 16, a["out"]), dict(t=torch.zeros(3), out=_bf(3, 16)),
                           [("t", torch.zeros(3, dtype=torch.float64), "dtype"), ("t", torch.zeros(6)[::2], "strided"),
                            ("out", _bf(3, 8), "count"), ("out", torch.zeros(3, 16), "dtype"), ("out", _bf(3, 32)[:, :16], "strided")]),
        "pad_mask": (lambda a: o.pad_mask(a["src"], a["offs"], 3, 5, 16, a["dst"], a["mask"], a["bias"], a["kvl"]), text,
                     text_bad + [("dst", _bf(14, 16), "count")]),
        "pack_mask": (lambda a: o.pack_mask(a["src"], a["offs"], 3, 5, 16, a["dst"], a["mask"], a["bias"], a["kvl"]), text,
                      text_bad + [("dst", _bf(15, 8), "width")]),
        "flow_mix": (lambda a: o.flow_mix(a["x"], a["noise"], a["sigma"], a["noisy"], a["target"]),
                     dict(x=_bf(2, 4, 3), noise=_bf(2, 4, 3), sigma=_bf(2), noisy=_bf(2, 4, 3), target=_bf(2, 4, 3)),
                     [("x", _bf(2, 4, 3).float(), "dtype"), ("x", _bf(2, 4, 6)[:, :, :3], "strided"), ("noise", _bf(2, 4, 2), "count"),
                      ("noise", _bf(2, 4, 3).float(), "dtype"), ("noisy", _bf(2, 4, 4), "count"), ("target", _bf(2, 3, 3), "count"),
                      ("target", _bf(2, 4, 6)[:, :, :3], "strided"), ("sigma", _bf(3), "count"), ("sigma", torch.zeros(2), "dtype")]),
        "mse_fwd_bwd": (lambda a: o.mse_fwd_bwd(a["pred"], a["target"], a["loss"], a["dpred"], a["ws"]),
                        dict(pred=_bf(2, 12), target=_bf(2, 12), loss=torch.zeros(1), dpred=_bf(2, 12), ws=torch.zeros(256)),
                        [("pred", _bf(2, 12).float(), "dtype"), ("pred", _bf(2, 24)[:, :12], "strided"), ("target", _bf(2, 11), "count"),
                         ("target", _bf(2, 12).float(), "dtype"), ("dpred", _bf(2, 13), "count"), ("dpred", _bf(2, 24)[:, :12], "strided"),
                         ("ws", torch.zeros(255), "count"), ("ws", torch.zeros(256, dtype=torch.float64), "dtype"),
                         ("loss", _bf(1), "dtype"), ("loss", torch.zeros(0), "count")]),
    }


NAMES = ["act_fwd", "act_bwd", "add_bf16", "f32_to_bf16", "transpose", "timestep_embed", "pad_mask", "pack_mask", "flow_mix",
         "mse_fwd_bwd"]


@pytest.mark.parametrize("name", NAMES)
def test_wrapper_rejects_before_any_library_call(ops, name):
    call, good, bad = _calls(ops)[name]
    with pytest.raises(ops.Reached):                                # well-formed arguments pass every check
        call(good)
    for arg, value, why in bad:
        with pytest.raises(ValueError):
            call({**good, arg: value})
    optional = {"act_fwd": ["y"], "act_bwd": ["dx"], "add_bf16": ["out"], "f32_to_bf16": ["y"], "transpose": ["out"],
                "timestep_embed": ["out"], "pad_mask": ["mask", "bias", "kvl"], "pack_mask": ["mask", "bias", "kvl"],
                "flow_mix": ["noisy", "target"], "mse_fwd_bwd": ["dpred"]}[name]
    for arg in optional:                                            # an absent optional operand is not an error
        with pytest.raises((ops.Reached, RuntimeError)):            # (torch.empty on "cpu" then reaches the tripwire)
            call({**good, arg: None})
