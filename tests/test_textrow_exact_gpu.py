"""The text-row kernels held to exact results at every lanes-per-row class, rows-per-block edge, residual variant and
layout -- GPU: yat_gemma_rmsnorm, yat_t5_rmsnorm, yat_dcae_rmsnorm_bias (csrc/rownorm_lpr.hpp), yat_clip_layernorm,
yat_rope_qk, yat_geglu, yat_embed_rows, yat_clip_embed.

Inputs and expectations come from tests/textrow_ref.py; test_textrow_ref_cpu.py proves their properties.  Norm outputs are
compared by bf16 bits (-0 counted as +0) over whole buffers that start as a canary (bits 0x7FC1) with guard rows around the
tensor.  rope_qk runs in place on a matrix whose v block and slack columns must come back bit for bit.  geglu's activation
was swept over every bf16 pattern by the glue pass; here its values are held to the fp64 reference through the module's two
roundings with that pass's bound, at separated gate / up views, ld > 2N, ldo > N, with guards.  The embeddings are held to
torch bit for bit.  One dense random case per norm epilogue with eps > 0 is held to close() at its defaults (the fp32 sum
order is not the reference's).
"""
import numpy as np
import pytest
import torch

from tests import glue_ref as G
from tests import textrow_ref as R
from tests.gpu_common import BF, DEV, _collect_failures, close  # noqa: F401

pytestmark = pytest.mark.gpu

CANARY = 0x7FC1
FAMILIES = ("pow4", "five")


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


def _bits(t):
    b = t.contiguous().view(torch.int16)
    return torch.where(b == -32768, torch.zeros_like(b), b)


def _canary(M, D, g0=2, g1=3):
    buf = torch.full((g0 + M + g1, D), CANARY, dtype=torch.int16, device=DEV).view(BF)
    return buf, buf[g0:g0 + M]


def _guarded(data, g0=2, g1=3):
    """an in/out operand inside canary rows -> (buffer, view)"""
    M, D = data.shape
    buf, view = _canary(M, D, g0, g1)
    view.copy_(data.to(DEV))
    return buf, view


def _same(fails, what, buf, want_rows, g0=2):
    """the whole buffer: canaries around the expected rows (fp32 / fp64 numpy, rounded once here as the store does)"""
    want = torch.full(buf.shape, CANARY, dtype=torch.int16).view(BF)
    want[g0:g0 + want_rows.shape[0]] = torch.from_numpy(np.ascontiguousarray(want_rows, dtype=np.float32)).to(BF)
    got, want = _bits(buf).cpu(), _bits(want)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, c = bad[0].tolist()
        fails.append(f"{what}: {bad.shape[0]} elements differ, first at buffer (row, col) ({r}, {c}): bits "
                     f"{got[r, c].item() & 0xffff:#06x}, expected {want[r, c].item() & 0xffff:#06x}")


def _dev(a):
    return R.to_bf(a).to(DEV)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", R.NORM_D)
def test_gemma_rmsnorm_exact(ops, D, family):
    fails = []
    for M in R.norm_rows(D):
        s, _, _ = R.rows(M, D, family, seed=D + M)
        w = R.weights(D, D, fine=True)
        res = R.coarse((M, D), D + M) * 8
        if family == "pow4":
            res = np.where(R.on_tie(R.expected_gemma(s, w, res).astype(np.float64)), 0.0, res)
        x, wd = _dev(s), _dev(w)
        buf, y = _canary(M, D)
        ops.gemma_rmsnorm(x, wd, y, eps=0.0)
        _same(fails, f"M={M} plain", buf, R.expected_gemma(s, w))
        buf, y = _canary(M, D)
        ops.gemma_rmsnorm(x, wd, y, eps=0.0, residual=_dev(res))
        _same(fails, f"M={M} residual apart", buf, R.expected_gemma(s, w, res))
        buf, y = _guarded(R.to_bf(res))
        ops.gemma_rmsnorm(x, wd, y, eps=0.0, residual=y)
        _same(fails, f"M={M} residual in place", buf, R.expected_gemma(s, w, res))
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", R.NORM_D)
def test_t5_rmsnorm_exact(ops, D, family):
    fails = []
    for M in R.norm_rows(D):
        s, _, _ = R.rows(M, D, family, seed=2 * D + M)
        w = R.weights(D, D + 1)
        x, res = R.split_residual(s, D + M)
        wd, want = _dev(w), R.expected_t5(s, w)
        buf, y = _canary(M, D)
        ops.t5_rmsnorm(_dev(s), wd, y, eps=0.0)
        _same(fails, f"M={M} plain", buf, want)
        buf, y = _canary(M, D)
        sbuf, sum_out = _canary(M, D)
        ops.t5_rmsnorm(_dev(x), wd, y, eps=0.0, residual=_dev(res), sum_out=sum_out)
        _same(fails, f"M={M} residual apart: y", buf, want)
        _same(fails, f"M={M} residual apart: sum", sbuf, s)
        buf, y = _canary(M, D)
        rbuf, r = _guarded(R.to_bf(res))
        ops.t5_rmsnorm(_dev(x), wd, y, eps=0.0, residual=r)
        _same(fails, f"M={M} sum_out is residual: y", buf, want)
        _same(fails, f"M={M} sum_out is residual: sum", rbuf, s)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", R.NORM_D)
def test_dcae_rmsnorm_bias_exact(ops, D, family):
    fails = []
    for M in R.norm_rows(D):
        s, _, _ = R.rows(M, D, family, seed=3 * D + M)
        w, b, res = R.coarse(D, D), R.coarse(D, D + 1), R.coarse((M, D), D + M)
        x, wd, bd = _dev(s), _dev(w), _dev(b)
        for bias, rr, relu, place in ((None, None, False, ""), (b, None, True, ""), (b, res, False, "apart"), (b, res, True, "in")):
            tag = f"M={M} bias={bias is not None} res={place} relu={relu}"
            want = R.expected_dcae(s, w, bias, rr, relu)
            if place == "in":
                buf, y = _guarded(R.to_bf(res))
                ops.dcae_rmsnorm_bias(x, wd, bd, y, eps=0.0, residual=y, relu=relu)
            else:
                buf, y = _canary(M, D)
                ops.dcae_rmsnorm_bias(x, wd, bd if bias is not None else None, y, eps=0.0,
                                      residual=_dev(rr) if rr is not None else None, relu=relu)
            _same(fails, tag, buf, want)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", R.NORM_D)
def test_clip_layernorm_exact(ops, D, family):
    fails = []
    for M in R.norm_rows(D):
        s, mu, _ = R.rows(M, D, family, seed=5 * D + M, centered=True)
        w, b = R.coarse(D, D + 2), R.coarse(D, D + 3)
        x, res = R.split_residual(s, D + M)
        wd, bd, want = _dev(w), _dev(b), R.expected_layernorm(s, mu, w, b)
        buf, y = _canary(M, D)
        ops.clip_layernorm(_dev(s), wd, bd, y, eps=0.0)
        _same(fails, f"M={M} plain", buf, want)
        buf, y = _canary(M, D)
        sbuf, sum_out = _canary(M, D)
        ops.clip_layernorm(_dev(x), wd, bd, y, eps=0.0, residual=_dev(res), sum_out=sum_out)
        _same(fails, f"M={M} residual apart: y", buf, want)
        _same(fails, f"M={M} residual apart: sum", sbuf, s)
        buf, y = _canary(M, D)
        rbuf, r = _guarded(R.to_bf(res))
        ops.clip_layernorm(_dev(x), wd, bd, y, eps=0.0, residual=r)
        _same(fails, f"M={M} sum_out is residual: y", buf, want)
        _same(fails, f"M={M} sum_out is residual: sum", rbuf, s)
    assert not fails, "; ".join(fails)


def test_norms_dense_random(ops):
    """eps > 0 on random data, one case per epilogue, against the module's formula in fp32 with its rounding points"""
    M, D = 37, 1544                                   # lpr 1: 193 chunks a lane
    g = torch.Generator().manual_seed(3)
    x, res = (torch.randn(M, D, generator=g).to(BF).to(DEV) for _ in range(2))
    w, b = ((torch.randn(D, generator=g) * 0.5).to(BF).to(DEV) for _ in range(2))

    def rb(t):
        return t.to(BF).float()
    n = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6)
    y = ops.gemma_rmsnorm(x, w, torch.empty_like(x), eps=1e-6)
    close(y, n * (1 + w.float()), "gemma")
    # (the residual sum is the kernel's own rounded norm output plus the residual, bit for bit: where the two nearly cancel, one
    # ulp of the norm output is many ulps of the sum, so the sum is not held to ulps of itself -- tests/test_gemma2_gpu.py)
    assert torch.equal(ops.gemma_rmsnorm(x, w, torch.empty_like(x), eps=1e-6, residual=res), res + y)
    s = rb(res.float() + x.float())
    ns = s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + 1e-6)
    close(ops.t5_rmsnorm(x, w, torch.empty_like(x), eps=1e-6, residual=res.clone()), w.float() * rb(ns), "t5")
    n5 = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    close(ops.dcae_rmsnorm_bias(x, w, b, torch.empty_like(x), eps=1e-5, residual=res, relu=True),
          torch.relu(rb(rb(rb(rb(n5) * w.float()) + b.float()) + res.float())), "dcae")
    close(ops.clip_layernorm(x, w, b, torch.empty_like(x), eps=1e-5, residual=res.clone()),
          torch.nn.functional.layer_norm(s, (D,), w.float(), b.float(), 1e-5), "clip layernorm")


# ---------------------------------------------------------------------------------------------------------------- rope_qk
@pytest.mark.parametrize("dh,heads,vheads,slack,lens", R.ROPE_CASES, ids=str)
def test_rope_qk_exact(ops, dh, heads, vheads, slack, lens):
    x, pos, cos, sin, ld = R.rope_case(dh, heads, vheads, slack, lens)
    assert (x.shape[0] * heads * (dh // 16)) % 256 != 0                     # the grid ends inside a block
    want = R.rope_ref(x, pos, cos, sin, heads, dh)
    buf, m = _guarded(R.to_bf(x))
    ops.rope_qk(m, heads, dh, torch.from_numpy(pos).to(DEV), _dev(cos), _dev(sin))
    fails = []
    _same(fails, "rope", buf, want)                                         # the v block and the slack: unchanged bit for bit
    assert not fails, fails[0]
    assert not np.array_equal(want[:, :heads * dh], x[:, :heads * dh])
    # a view of a wider matrix (ld > the width): the columns outside the view stay as they were
    wide = torch.full((x.shape[0] + 2, ld + 16), CANARY, dtype=torch.int16, device=DEV).view(BF)
    wide[1:-1, 8:8 + ld] = R.to_bf(x).to(DEV)
    wantw = wide.clone()
    wantw[1:-1, 8:8 + ld] = R.to_bf(want).to(DEV)
    ops.rope_qk(wide[1:-1, 8:8 + ld], heads, dh, torch.from_numpy(pos).to(DEV), _dev(cos), _dev(sin))
    assert torch.equal(_bits(wide), _bits(wantw))


# ------------------------------------------------------------------------------------------------------------------ geglu
@pytest.mark.parametrize("M,N,pad,opad", R.GEGLU_CASES, ids=str)
def test_geglu_layouts(M, N, pad, opad):
    import ctypes
    from yat_amd import lib
    gate, up = R.geglu_case(M, N)
    ld, ldo = 2 * N + 2 * pad + 8, N + opad
    buf = torch.full((M + 2, ld), 32768.0, dtype=BF)
    buf[1:-1, 8 + pad + N:8 + pad + 2 * N] = gate                           # up | gap | gate: separated views, gate second
    buf[1:-1, 8:8 + N] = up
    buf = buf.to(DEV)
    out = torch.full((M + 2, ldo), CANARY, dtype=torch.int16, device=DEV).view(BF)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(t, e):
        return ctypes.c_void_p(t.data_ptr() + 2 * e)
    assert lib.load().yat_geglu(M, N, p(buf, ld + 8 + pad + N), p(buf, ld + 8), ld, p(out, ldo), ldo, st) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    keep = torch.full((M + 2, ldo), CANARY, dtype=torch.int16)
    assert torch.equal(got[0].view(torch.int16), keep[0]) and torch.equal(got[-1].view(torch.int16), keep[-1])
    assert torch.equal(got[1:-1, N:].view(torch.int16), keep[1:-1, N:])
    g64 = G.ref_f64("gelu_tanh", gate.double().numpy())
    u = up.double().numpy()
    eg = (0.5 + G.act_margin()) * G.ulp_bf16(g64) + G.ACT_ABS              # the inner rounding, the glue pass's bound
    bound = eg * np.abs(u) + 0.5 * G.ulp_bf16(np.abs(g64 * u) + eg * np.abs(u))
    err = np.abs(got[1:-1, :N].double().numpy() - g64 * u)
    assert (err <= bound).all(), float((err - bound).max())
    exact = (gate.float() >= 9) | (gate.float() == 0) | (gate.float() <= -30)      # gelu(x) = x or +-0 in fp32: an exact product
    want = (torch.where(gate.float() > 0, gate.float(), torch.zeros(())) * up.float()).to(BF)
    assert torch.equal(_bits(got[1:-1, :N][exact]), _bits(want[exact]))


# ------------------------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("nrows,D,vocab", R.EMBED_CASES, ids=str)
def test_embeddings_equal_torch(ops, nrows, D, vocab):
    c = R.embed_case(nrows, D, vocab, npos=vocab + 2)
    table, ids, ptab, pos = (c[n].to(DEV) for n in ("table", "ids", "ptab", "pos"))
    for scale in (1.0, 0.25, float(torch.tensor(float(D) ** 0.5).to(BF))):
        buf, out = _canary(nrows, D)
        ops.embed_rows(ids, table, scale, out)
        want = (table[ids.long()].float() * scale).to(BF)
        assert torch.equal(_bits(out), _bits(want)), scale
        assert (buf[:2].view(torch.int16) == CANARY).all() and (buf[2 + nrows:].view(torch.int16) == CANARY).all()
    buf, out = _canary(nrows, D)
    ops.clip_embed(ids, pos, table, ptab, out)
    assert torch.equal(_bits(out), _bits((table[ids.long()].float() + ptab[pos.long()].float()).to(BF)))
    assert (buf[:2].view(torch.int16) == CANARY).all() and (buf[2 + nrows:].view(torch.int16) == CANARY).all()
