"""The "glue" kernels (csrc/elementwise.hip, csrc/pixart_ops.hip, the row routing of csrc/mmdit_ops.hip) held to exact
results at every grid wrap, chunk pass and edge -- GPU.

Inputs, plain references and the case lists come from tests/glue_ref.py; test_glue_ref_cpu.py proves that the lists reach
every launch class and that the expected bits need no device arithmetic.  Nothing is compared with another run of a
kernel.  Every output sits in a buffer that starts as a canary (bf16 bits 0x7FC1) and is compared whole, on bits; -0 and
+0 count as equal where arithmetic produced the value, copies are compared raw.  Each test collects all its mismatches
before it fails.

test_activation_sweep sends every bf16 bit pattern through act_fwd and act_bwd (dy = 1 and dy = -3) and bounds the result
by (0.5 + m) bf16 ulps + 2^-30 of a cancellation-free fp64 reference, with m = 8 x the excess of the numpy fp32 model of
the same formulas (0.023, test_glue_ref_cpu.py), on every finite input on which torch's own fp32 CPU result is finite.
Measured on an MI355X, largest distance in bf16 ulps (bound 0.5231): silu 0.5000, gelu_tanh 0.4998, dsilu 0.5000 (dy = -3:
0.5000), dgelu_tanh 0.4999 (dy = -3: 0.4998) -- the final rounding is all there is.  Before dgelu_tanh_f kept -inf out of
its product with s = 0 the device returned NaN on the 10838 finite inputs x <= -1.168e13, on 2646 of which (down to
-1.8e19) torch is finite; every other finite input kept its bits (profiles/glue_exact_a_act_sweep.txt).
"""
import hashlib

import numpy as np
import pytest
import torch

from tests import glue_ref as R
from tests.gpu_common import BF, DEV, _collect_failures, close  # noqa: F401  (the autouse fixture close() reports through)

pytestmark = pytest.mark.gpu
I16, F32 = torch.int16, torch.float32
TAIL = 24                                # canary elements behind a flat output


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


# ------------------------------------------------------------------------------------------------ buffers
def flat_out(n, dtype=BF):
    """(buffer, view of its first n elements): canaries, n of them to be written by a kernel"""
    if dtype == BF:
        buf = torch.full((n + TAIL,), R.CANARY, dtype=I16, device=DEV).view(BF)
    else:
        buf = torch.full((n + TAIL,), 12345, dtype=dtype, device=DEV)
    return buf, buf[:n]


def flat_want(bits, fold=True):
    """the bits of a whole flat bf16 buffer: ``bits`` (int16, CPU), then the canary tail"""
    bits = bits.reshape(-1)
    return torch.cat([R.fold(bits) if fold else bits, torch.full((TAIL,), R.CANARY, dtype=I16)])


def check(fails, what, buf, want, fold=True):
    """``buf`` (device, bf16 or int16, any shape) against ``want`` (CPU int16 bits of the same shape)"""
    got = buf.view(I16).cpu() if buf.dtype == BF else buf.cpu()
    got = R.fold(got) if fold else got
    want = want.reshape(got.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        at = tuple(bad[0].tolist())
        fails.append(f"{what}: {bad.shape[0]} elements differ, first at {at}: bits {got[at].item() & 0xffff:#06x}, "
                     f"expected {want[at].item() & 0xffff:#06x}")


def check_same(fails, what, got, want):
    """non-bf16 outputs (mask, key bias, kv_len, rstd tails): whole tensors, by value"""
    if not torch.equal(got.cpu(), want):
        fails.append(f"{what}: {(got.cpu() != want).sum().item()} elements differ")


def window(rows, cols, pad, c0, r0, r1, data=None):
    """(buffer [r0 + rows + r1, cols + pad] int16, view [rows, cols] as bf16): ``data`` (int16 bits, CPU) inside guards,
    or canaries to be written by a kernel; the view starts at row r0 and at the nonzero column c0"""
    fill = R.CANARY if data is None else R.GUARD
    buf = torch.full((r0 + rows + r1, cols + pad), fill, dtype=I16, device=DEV)
    if data is not None:
        buf[r0:r0 + rows, c0:c0 + cols] = data.to(DEV)
    return buf, buf.view(BF)[r0:r0 + rows, c0:c0 + cols]


def window_want(rows, cols, pad, c0, r0, r1, bits):
    """the bits of a whole output buffer: canaries around ``bits``"""
    want = torch.full((r0 + rows + r1, cols + pad), R.CANARY, dtype=I16)
    want[r0:r0 + rows, c0:c0 + cols] = bits
    return want


# ------------------------------------------------------------------------------------------------ ew_kernel
@pytest.mark.parametrize("n", R.EW_N)
def test_ew_kernel(ops, n):
    """act_fwd and act_bwd of both activations on saturated integers (x or 0; dy or 0), and add_bf16 on small integers"""
    fails = []
    x, dy, fwd, bwd = R.ew_case(n)
    xd, dyd = x.to(DEV), dy.to(DEV)
    for act in R.ACTS:
        buf, y = flat_out(n)
        ops.act_fwd(xd, act, y)
        check(fails, f"act_fwd {act}", buf, flat_want(fwd))
        buf, dx = flat_out(n)
        ops.act_bwd(xd, dyd, act, dx)
        check(fails, f"act_bwd {act}", buf, flat_want(bwd))
    a, b, want = R.add_case(n)
    buf, out = flat_out(n)
    ops.add_bf16(a.to(DEV), b.to(DEV), out)
    check(fails, "add_bf16", buf, flat_want(want))
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ activation sweep
def _digest(bits, sel):
    return hashlib.sha256(bits.numpy()[sel].tobytes()).hexdigest()[:16]


def test_activation_sweep(ops):
    fails = []
    bits, x = R.all_bf16()
    xd = bits.to(DEV).view(BF)
    fin, m = np.isfinite(x), R.act_margin()
    ones, m3 = torch.ones(65536, dtype=BF, device=DEV), torch.full((65536,), -3.0, dtype=BF, device=DEV)
    outside_band = ~(x <= np.float32(-1.16e13))
    for act in R.ACTS:
        for name, dy, run in ((act, 1.0, lambda: ops.act_fwd(xd, act)), ("d" + act, 1.0, lambda: ops.act_bwd(xd, ones, act)),
                              ("d" + act, -3.0, lambda: ops.act_bwd(xd, m3, act))):
            out_bits = run().view(I16).cpu()
            out = out_bits.view(BF).double().numpy()
            ref = dy * R.ref_f64(name, x)
            tor = R.torch_f32(name, x)
            dom = fin & np.isfinite(tor) & (np.abs(ref) <= R.BF16_MAX)
            tag = f"{name} dy={dy:g}"
            if not np.isnan(out[np.isnan(x)]).all():
                fails.append(f"{tag}: a NaN input gave a number")
            lost = dom & ~np.isfinite(out)
            if lost.any():
                fails.append(f"{tag}: not finite on {lost.sum()} inputs where torch's fp32 result is, x in "
                             f"[{x[lost].min():g}, {x[lost].max():g}]")
            ok = dom & np.isfinite(out)
            with np.errstate(all="ignore"):
                dist = np.where(ok, (np.abs(out - ref) - R.ACT_ABS) / R.ulp_bf16(ref), 0.0)
            k = int(np.argmax(dist))
            print(f"[sweep] {tag}: at most {max(dist[k], 0):.4f} bf16 ulps from the fp64 reference (x = {x[k]:g}; bound "
                  f"{0.5 + m:.4f}); x = -inf -> {out[x == -np.inf][0]:g}, +inf -> {out[x == np.inf][0]:g}; sha256 of the "
                  f"bits outside x <= -1.16e13: {_digest(out_bits, outside_band)}, of all: {_digest(out_bits, slice(None))}; "
                  f"NaN outputs on finite inputs: {int((fin & np.isnan(out)).sum())}")
            if not dist[k] <= 0.5 + m:
                fails.append(f"{tag}: {dist[k]:.4f} bf16 ulps from the reference at x = {x[k]:g} (bound {0.5 + m:.4f}), "
                             f"{int((dist > 0.5 + m).sum())} inputs beyond the bound")
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ f32_to_bf16
@pytest.mark.parametrize("n", ["table"] + R.F32_N)
def test_f32_to_bf16(ops, n):
    """every upper half x six lower halves (ties, carries into the exponent, overflow to inf, denormals), expectation from
    integer arithmetic; a NaN stays a NaN, its payload is free"""
    u, r, nan = R.rne_table() if n == "table" else R.rne_case(n)
    buf, y = flat_out(len(u))
    ops.f32_to_bf16(torch.from_numpy(u.view(np.int32).copy()).to(DEV).view(F32), y)
    got = buf.view(I16).cpu()
    fails = []
    if not got[len(u):].eq(R.CANARY).all():
        fails.append("wrote behind the output")
    g = got[:len(u)].numpy().view(np.uint16)
    if not np.array_equal(g[~nan], r[~nan]):
        bad = np.nonzero(g[~nan] != r[~nan])[0]
        fails.append(f"{len(bad)} finite inputs round wrong, first {u[~nan][bad[0]]:#010x} -> {g[~nan][bad[0]]:#06x}, expected "
                     f"{r[~nan][bad[0]]:#06x}")
    if not (((g[nan] & 0x7F80) == 0x7F80) & ((g[nan] & 0x7F) != 0)).all():
        fails.append("a NaN input gave a number")
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ flow_mix / ddpm
@pytest.mark.parametrize("B,per", R.FLOW_CASES)
def test_flow_mix(ops, B, per):
    x, nz, sig, _ = R.mix_case(B, per)
    noisy_w, target_w = R.flow_ref(x, nz, sig)
    (nbuf, noisy), (tbuf, target) = flat_out(B * per), flat_out(B * per)
    ops.flow_mix(x.to(DEV), nz.to(DEV), sig.to(DEV), noisy.view(B, per), target.view(B, per))
    fails = []
    check(fails, "noisy", nbuf, flat_want(R.bf_bits(noisy_w)))
    check(fails, "target", tbuf, flat_want(R.bf_bits(target_w)))
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("B,per", R.DDPM_CASES)
def test_ddpm_add_noise(ops, B, per):
    x, nz, ca, cb = R.mix_case(B, per, seed=5)
    buf, noisy = flat_out(B * per)
    ops.ddpm_add_noise(x.to(DEV), nz.to(DEV), ca.to(DEV), cb.to(DEV), noisy.view(B, per))
    fails = []
    check(fails, "noisy", buf, flat_want(R.bf_bits(R.ddpm_ref(x, nz, ca, cb))))
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ mse
@pytest.mark.parametrize("n", R.MSE_N)
def test_mse_fwd_bwd(ops, n):
    """integer differences: the sum of squares is exact in any order.  n and gscale powers of two: loss and dpred exact;
    else loss within 2 fp32 ulps of the fp64 S / n and dpred within 1 bf16 ulp of the fp64 2 gscale d / n"""
    pred, target, d, S = R.mse_case(n)
    pd, td = pred.to(DEV), target.to(DEV)
    fails = []
    for gscale in R.MSE_GSCALE:
        for with_dpred in (True, False):
            ws = torch.full((256 + TAIL,), float("nan"), device=DEV)
            ws[256:] = 12345.0
            loss = torch.full((1 + TAIL,), 12345.0, device=DEV)
            dbuf, dpred = flat_out(n)
            ops.mse_fwd_bwd(pd, td, loss[:1], dpred if with_dpred else None, ws[:256], gscale=gscale)
            tag = f"gscale {gscale} {'with' if with_dpred else 'without'} dpred"
            if not (ws[256:] == 12345.0).all() or not (loss[1:] == 12345.0).all():
                fails.append(f"{tag}: wrote behind the workspace or the loss")
            got, want = loss[0].item(), S / n
            dist = abs(got - want) / R.ulp32(want)
            exact = R.pow2(n) and R.pow2(gscale)
            print(f"[mse] n={n} {tag}: loss {dist:.2f} fp32 ulps from S / n")
            if not dist <= (0 if exact else 2):
                fails.append(f"{tag}: loss {got!r}, expected {want!r} ({dist:.2f} fp32 ulps)")
            if not with_dpred:
                check(fails, f"{tag}: dpred buffer", dbuf, torch.full((n + TAIL,), R.CANARY, dtype=I16))
                continue
            g64 = 2.0 * gscale * d.astype(np.float64) / n
            if exact:
                check(fails, f"{tag}: dpred", dbuf, flat_want(R.bf_bits(torch.from_numpy(g64).to(BF))))
            else:
                gb = dbuf.view(I16).cpu()
                if not gb[n:].eq(R.CANARY).all():
                    fails.append(f"{tag}: wrote behind dpred")
                err = np.abs(gb[:n].view(BF).double().numpy() - g64) / R.ulp_bf16(g64)
                if not err.max() <= 1:
                    fails.append(f"{tag}: dpred {err.max():.2f} bf16 ulps from 2 gscale d / n at element {int(err.argmax())}")
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("real", [False, True], ids=["integers", "real"])
@pytest.mark.parametrize("B,used,stride", R.MSE_CHUNK)
def test_mse_bf16_chunk(ops, B, used, stride, real):
    """integers: loss and dpred exact.  real values: dpred equals the fp32 restatement with a bf16 rounding after each op;
    the loss (an fp32 sum in another order, then rounded to bf16) is a bf16 number within 0.5 + 2^-6 bf16 ulps of the
    restatement's fp64 mean.  The dpred of the unused half is exact zeros."""
    pred, target = R.chunk_case(B, used, stride, real)
    fails = []
    for gscale in (1.0, 0.3):
        dp_w, S, loss_w = R.chunk_ref(pred, target, gscale)
        ws = torch.full((256 + TAIL,), float("nan"), device=DEV)
        ws[256:] = 12345.0
        loss = torch.full((1 + TAIL,), 12345.0, device=DEV)
        dbuf, dpred = flat_out(B * stride)
        ops.mse_bf16_chunk(pred.to(DEV).view(B, stride, 1, 1), target.to(DEV).view(B, used, 1, 1), loss[:1],
                           dpred.view(B, stride, 1, 1), ws[:256], gscale=gscale)
        if not (ws[256:] == 12345.0).all() or not (loss[1:] == 12345.0).all():
            fails.append(f"gscale {gscale}: wrote behind the workspace or the loss")
        check(fails, f"gscale {gscale}: dpred", dbuf, flat_want(R.bf_bits(dp_w)))
        got, v = loss[0].item(), S / (B * used)
        # real values: the fp32 sum runs in another order -- a tree of at most 24 additions per element and two more
        # roundings, below 2^-19 relative, 2^-11 bf16 ulps; 2^-6 on top of the final rounding's half ulp holds that
        if not (abs(got - v) <= (0.5 + 2.0 ** -6) * float(R.ulp_bf16(v)) if real else got == loss_w):
            fails.append(f"gscale {gscale}: loss {got!r}, expected {loss_w!r} = bf16({v!r})")
        if got != float(torch.tensor(got).to(BF)):
            fails.append(f"gscale {gscale}: loss {got!r} is not a bf16 number")
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("n", R.DROP_N)
def test_dropout(ops, n):
    """forward and backward_add against the splitmix64 mask computed in numpy, for every p and seed"""
    x, g, io0 = R.drop_inputs(n)
    xd, gd = x.to(DEV), g.to(DEV)
    fails = []
    for p in R.DROP_P:
        for seed in R.DROP_SEEDS:
            keep = R.drop_keep(seed, n, p)
            y_w, _ = R.drop_ref(x, io0, keep, p)
            _, io_w = R.drop_ref(g, io0, keep, p)
            buf, y = flat_out(n)
            ops.dropout(xd, p, seed, y)
            check(fails, f"p={p!r} seed={seed}: forward ({int(keep.sum())} of {n} kept)", buf, flat_want(R.bf_bits(y_w)))
            buf, io = flat_out(n)
            io.copy_(io0)
            ops.dropout_bwd_add(gd, p, seed, io)
            check(fails, f"p={p!r} seed={seed}: backward_add", buf, flat_want(R.bf_bits(io_w)))
    assert not fails, "; ".join(fails[:6])


# ------------------------------------------------------------------------------------------------ pad_mask / pack_mask
def _text_run(ops, fails, tag, B, T, C, lens, rows_padded):
    src, offs, dst_w, mask_w, bias_w, kvl_w = R.text_case(B, T, C, lens, rows_padded)
    rows = B * T if rows_padded is None else rows_padded
    srcd, offd = src.to(DEV).view(BF), offs.to(DEV)
    for absent in (None, "mask", "bias", "kvl"):
        dbuf = torch.full((rows + 2, C), R.CANARY, dtype=I16, device=DEV)
        mask, _ = flat_out(B * T, torch.int64)
        bias, _ = flat_out(B * T, F32)
        kvl, _ = flat_out(B, torch.int32)
        args = [None if absent == "mask" else mask[:B * T], None if absent == "bias" else bias[:B * T],
                None if absent == "kvl" else kvl[:B]]
        if rows_padded is None:
            ops.pad_mask(srcd, offd, B, T, C, dbuf.view(BF)[:rows], *args)
        else:
            ops.pack_mask(srcd, offd, B, T, C, dbuf.view(BF)[:rows], *args)
        t = f"{tag} without {absent}" if absent else tag
        check(fails, f"{t}: dst", dbuf, torch.cat([dst_w, torch.full((2, C), R.CANARY, dtype=I16)]), fold=False)
        for name, got, want in (("mask", mask, mask_w), ("bias", bias, bias_w), ("kvl", kvl, kvl_w)):
            tail = torch.full((TAIL,), 12345, dtype=want.dtype)
            body = torch.full_like(want, 12345) if absent == name else want
            check_same(fails, f"{t}: {name}", got, torch.cat([body, tail]))


@pytest.mark.parametrize("C", R.TEXT_C)
def test_pad_mask(ops, C):
    fails = []
    for B, T, lens in R.TEXT_BT:
        _text_run(ops, fails, f"B={B} T={T} lens={lens}", B, T, C, lens, None)
    assert not fails, "; ".join(fails[:6])


@pytest.mark.parametrize("C", R.TEXT_C)
def test_pack_mask(ops, C):
    fails = []
    for B, T, lens in R.TEXT_BT:
        for rp in R.pack_rows_padded(B, T, lens):
            _text_run(ops, fails, f"B={B} T={T} lens={lens} rows_padded={rp}", B, T, C, lens, rp)
    assert not fails, "; ".join(fails[:6])


# ------------------------------------------------------------------------------------------------ patch_rearrange
@pytest.mark.parametrize("B,C,H,W,p", R.PATCH_CASES)
def test_patch_rearrange(ops, B, C, H, W, p):
    """both directions and both column orders against the plain permutation, and the round trip"""
    n = B * C * H * W
    img = R.pattern(n, 11).view(B, C, H, W)
    imgd = img.to(DEV).view(BF)
    fails = []
    for cm in (True, False):
        tok_w = R.patch_ref(img, p, cm)
        buf, tok = flat_out(n)
        ops.patch_rearrange(imgd, tok.view(tok_w.shape), B, C, H, W, p, cm, True)
        check(fails, f"to tokens, channel_major={cm}", buf, flat_want(tok_w, fold=False), fold=False)
        # from tokens: the tokens are a fresh pattern, the image its inverse permutation
        tok2 = R.pattern(n, 777).view(tok_w.shape)
        idx = R.patch_ref(torch.arange(n, dtype=torch.int64).view(B, C, H, W), p, cm).reshape(-1)
        img_w = torch.empty(n, dtype=I16)
        img_w[idx] = tok2.reshape(-1)
        if not cm:
            assert torch.equal(img_w.view(B, C, H, W), R.unpatchify_ref(tok2, B, C, H, W, p))     # "nhwpqc->nchpwq"
        buf, back = flat_out(n)
        ops.patch_rearrange(tok2.to(DEV).view(BF), back.view(B, C, H, W), B, C, H, W, p, cm, False)
        check(fails, f"from tokens, channel_major={cm}", buf, flat_want(img_w, fold=False), fold=False)
        buf, rt = flat_out(n)                                       # round trip of what the kernel itself wrote
        ops.patch_rearrange(tok.view(tok_w.shape), rt.view(B, C, H, W), B, C, H, W, p, cm, False)
        check(fails, f"round trip, channel_major={cm}", buf, flat_want(img, fold=False), fold=False)
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ add_pos_embed
@pytest.mark.parametrize("rows,N,D", R.POS_CASES)
def test_add_pos_embed(ops, rows, N, D):
    """integers + (k + 0.5): the fp32 sum is exact and mostly a tie between two bf16 numbers; out of place and in place"""
    x, pos, want, _ = R.pos_case(rows, N, D)
    posd = pos.to(DEV)
    fails = []
    buf, out = flat_out(rows * D)
    ops.add_pos_embed(x.to(DEV), posd, out.view(rows, D))
    check(fails, "out of place", buf, flat_want(R.bf_bits(want)))
    buf, io = flat_out(rows * D)
    io.copy_(x.reshape(-1))
    ops.add_pos_embed(io.view(rows, D), posd)
    check(fails, "in place", buf, flat_want(R.bf_bits(want)))
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ joint_rows
JL = dict(joint=(8, 8, 1, 2), img=(24, 16, 2, 1), txt=(40, 8, 1, 1))      # (pad, first column, rows before, rows after)


@pytest.mark.parametrize("B,N,T,C", R.JOINT_CASES)
def test_joint_rows(ops, B, N, T, C):
    """every operand a window of its own canary buffer, nonzero first column, three different leading dimensions"""
    img, txt, joint = R.joint_case(B, N, T, C)
    L = N + T
    big = B * L * C > 1 << 22
    fails = []
    text_rows = torch.zeros(B, L, dtype=torch.bool)
    text_rows[:, N:] = True
    text_rows = text_rows.view(-1)
    _, img_in = window(B * N, C, *JL["img"], data=img)
    _, txt_in = window(B * T, C, *JL["txt"], data=txt) if T else (None, None)
    _, joint_in = window(B * L, C, *JL["joint"], data=joint)
    # to joint
    jbuf, jv = window(B * L, C, *JL["joint"])
    ops.joint_rows(jv, img_in, txt_in, B, N, T, to_joint=True)
    check(fails, "to joint", jbuf, window_want(B * L, C, *JL["joint"], joint), fold=False)
    if T and not big:                                               # no text side: its rows become zeros
        jbuf, jv = window(B * L, C, *JL["joint"])
        ops.joint_rows(jv, img_in, None, B, N, T, to_joint=True)
        z = joint.clone()
        z[text_rows] = 0
        check(fails, "to joint, txt None", jbuf, window_want(B * L, C, *JL["joint"], z), fold=False)
    # from joint
    ibuf, iv = window(B * N, C, *JL["img"])
    tbuf, tv = window(B * T, C, *JL["txt"]) if T else (None, None)
    ops.joint_rows(joint_in, iv, tv, B, N, T, to_joint=False)
    check(fails, "from joint: img", ibuf, window_want(B * N, C, *JL["img"], img), fold=False)
    if T:
        check(fails, "from joint: txt", tbuf, window_want(B * T, C, *JL["txt"], txt), fold=False)
    if T and not big:                                               # no text side: only the image rows are written
        ibuf, iv = window(B * N, C, *JL["img"])
        tbuf, _ = window(B * T, C, *JL["txt"])
        ops.joint_rows(joint_in, iv, None, B, N, T, to_joint=False)
        check(fails, "from joint, txt None: img", ibuf, window_want(B * N, C, *JL["img"], img), fold=False)
        check(fails, "from joint, txt None: txt keeps its canary", tbuf, torch.full(tuple(tbuf.shape), R.CANARY, dtype=I16), fold=False)
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ qknorm_concat
QL = dict(img=(24, 8, 1, 2), txt=(40, 16, 2, 1), joint=(8, 8, 1, 1), dj=(56, 24, 1, 2), dimg=(16, 8, 2, 1), dtxt=(32, 16, 1, 1))
assert len({v[0] for v in QL.values()}) == 6


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


@pytest.mark.parametrize("B,N,T,H,dh", R.QKNORM_CASES)
def test_qknorm_concat(ops, B, N, T, H, dh):
    """six different leading dimensions above 3D, canaries around joint, dimg and dtxt; the v section and the row routing by
    bits, q | k against the bf16 restatement (bit-identical; the inputs keep every normalised element 2^-9 bf16 ulps from
    a tie, so the expectation does not hang on the order of an fp32 sum -- on plain randn 2 of 131,840 elements of the
    second case sat on a tie and came out one bf16 step from torch's CPU bits), dx and dw against fp32 autograd with the
    bounds of test_sd3_gpu.py::test_qknorm_concat_fwd_bwd; rstd against the fp64 statistics"""
    D, L, eps = H * dh, N + T, R.QKNORM_EPS
    W3 = 3 * D
    fails = []
    qi, qt = R.qknorm_inputs(B * N, D, 1, 5, dh), (R.qknorm_inputs(B * T, D, 2, 30000, dh) if T else None)
    dj = R.qknorm_inputs(B * L, D, 5, 50000)
    ws = [(1.0 + 0.2 * torch.randn(dh, generator=torch.Generator().manual_seed(10 + k))).to(BF) for k in range(4)]
    wsd = [w.to(DEV) for w in ws]
    _, img = window(B * N, W3, *QL["img"], data=R.bf_bits(qi))
    _, txt = window(B * T, W3, *QL["txt"], data=R.bf_bits(qt)) if T else (None, None)
    jbuf, joint = window(B * L, W3, *QL["joint"])
    rstd = torch.full((B * L * 2 * H + TAIL,), 12345.0, device=DEV)
    rs = rstd[:B * L * 2 * H].view(B * L, 2 * H)
    ops.qknorm_concat_fwd(img, txt, B, N, T, H, dh, eps, wsd[0], wsd[1], wsd[2] if T else None, wsd[3] if T else None, joint, rs)
    # q | k: the restatement on the real-valued sections; v: the routing of the copy pattern
    zero_v = lambda t: None if t is None else torch.cat([t[:, :2 * D], torch.zeros_like(t[:, 2 * D:])], 1)
    o_bf, _, _ = R.qknorm_concat_ref(zero_v(qi), zero_v(qt), wsd, B, N, T, H, dh, eps, BF)
    want = R.bf_bits(o_bf.detach())
    vi, vt = R.bf_bits(qi)[:, 2 * D:].view(B, N, D), (R.bf_bits(qt)[:, 2 * D:].view(B, T, D) if T else torch.zeros(B, 0, D, dtype=I16))
    want[:, 2 * D:] = torch.cat([vi, vt], 1).reshape(B * L, D)
    got = jbuf.cpu()
    want_buf = window_want(B * L, W3, *QL["joint"], want)
    pad, c0, r0, r1 = QL["joint"]
    qk = torch.zeros_like(got, dtype=torch.bool)
    qk[r0:r0 + B * L, c0:c0 + 2 * D] = True                         # arithmetic there: -0 = +0; raw bits everywhere else
    got_f, want_f = torch.where(qk, R.fold(got), got), torch.where(qk, R.fold(want_buf), want_buf)
    check(fails, "joint", got_f, want_f, fold=False)
    if not (rstd[B * L * 2 * H:] == 12345.0).all():
        fails.append("wrote behind rstd")
    x64 = torch.cat([qi.view(B, N, 3, H, dh)[:, :, :2]] + ([qt.view(B, T, 3, H, dh)[:, :, :2]] if T else []), 1).double()
    rs64 = torch.rsqrt(x64.pow(2).mean(-1) + eps).reshape(B * L, 2 * H)
    e = ((rs.cpu().double() - rs64).abs() / rs64).max().item()
    if not e <= (dh + 8) * 2.0 ** -24:                              # dh fp32 additions, the mean, eps, rsqrtf
        fails.append(f"rstd {e:.3e} relative from the fp64 statistics")
    # backward
    _, djv = window(B * L, W3, *QL["dj"], data=R.bf_bits(dj))
    ibuf, dimg = window(B * N, W3, *QL["dimg"])
    tbuf, dtxt = window(B * T, W3, *QL["dtxt"]) if T else (None, None)
    dws = [torch.zeros(dh, dtype=BF, device=DEV) for _ in range(4)]
    wsb = torch.empty(ops.qknorm_concat_bwd_workspace_bytes(B, N, T, dh), dtype=torch.uint8, device=DEV)
    ops.qknorm_concat_bwd(img, txt, B, N, T, H, dh, wsd[0], wsd[1], wsd[2] if T else None, wsd[3] if T else None, rs, djv,
                          dimg, dtxt, dws[0], dws[1], dws[2] if T else None, dws[3] if T else None, wsb)
    o32, parts, w32 = R.qknorm_concat_ref(zero_v(qi), zero_v(qt), wsd, B, N, T, H, dh, eps, torch.float32)
    o32.backward(zero_v(dj).float())
    djb = R.bf_bits(dj).view(B, L, W3)
    for name, buf, rows, per, lay, part, lo in (("dimg", ibuf, B * N, N, QL["dimg"], parts[0], 0),
                                                ("dtxt", tbuf, B * T, T, QL["dtxt"], parts[1] if T else None, N)):
        if buf is None:
            continue
        pad, c0, r0, r1 = lay
        g = buf.cpu()
        v_w = djb[:, lo:lo + per, 2 * D:].reshape(rows, D)          # d_v: the joint rows of this stream, routed back
        w_buf = window_want(rows, W3, *lay, torch.cat([g[r0:r0 + rows, c0:c0 + 2 * D], v_w], 1))
        check(fails, f"{name}: v section and canaries", g, w_buf, fold=False)
        e = _rel(g[r0:r0 + rows, c0:c0 + 2 * D].view(BF), part.grad.reshape(rows, 3, D)[:, :2].reshape(rows, 2 * D))
        print(f"[qknorm] {name} rel={e:.3e}")
        if not e <= R.QKNORM_DX_REL:
            fails.append(f"{name}: rel l2 {e:.3e} > {R.QKNORM_DX_REL}")
    for k in range(4 if T else 2):
        ek = _rel(dws[k], w32[k].grad)
        if not ek <= R.QKNORM_DW_REL:
            fails.append(f"dw[{k}]: rel l2 {ek:.3e} > {R.QKNORM_DW_REL}")
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------ timestep_embed
@pytest.mark.parametrize("B,dim", R.TSTEP_CASES)
def test_timestep_embed(ops, B, dim):
    """t = 0 gives exactly [1 ... | 0 ...]; other t within the bounds of test_kernels_gpu.py::test_timestep_embed of the
    fp64 cos / sin; canaries behind the output"""
    t = R.TSTEP_T[:B]
    buf, out = flat_out(B * dim)
    ops.timestep_embed(torch.tensor(t, dtype=F32, device=DEV), dim, out.view(B, dim))
    got = buf.view(I16).cpu()
    assert got[B * dim:].eq(R.CANARY).all(), "wrote behind the output"
    o = got[:B * dim].view(BF).view(B, dim)
    half = dim // 2
    assert t[0] == 0.0 and torch.equal(o[0].float(), torch.cat([torch.ones(half), torch.zeros(half)]))
    close(o, R.tstep_ref(t, dim), f"timestep_embed B={B} dim={dim}", tol=3e-3, ulps=2, atol=2e-3)
