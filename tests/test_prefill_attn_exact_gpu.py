"""The forward-only prefill attention kernels (csrc/attn_prefill.hpp and its users: vae_attn_kernel<64|512>,
gemma_attn_kernel<8,8|4,4|4,2|4,1>, t5_attn_kernel, clip_attn_kernel) held to exact results at every instantiation, prompt
length class, batch shape, offset and leading dimension -- GPU.

Inputs, the plain fp64 reference and the case lists come from tests/prefill_attn_ref.py; test_prefill_attn_ref_cpu.py proves
that every score is an exact fp32 integer, that the softmax weights are exactly 1/g or 0 (selector and bias-only cases) or
powers of two with a power-of-two sum (ladder cases), that the expected output is exact in bf16 or rounded once from an exact
fp32 value, and that the lists reach every class.  So the kernels must store the bits the reference rounds to, and every
comparison here is equality of bf16 bits (-0 counted as +0) over the WHOLE output buffer.  Nothing is compared with another
run of a kernel.

  * The library entry points are called directly (``lib.load().yat_*_attn_fwd``), which frees the offsets and leading
    dimensions: cases alternate between [q | k | v] at ld = width and  v | gap | q | gap | k | slack  with ld and ldo wider than
    the width and ``out`` at a nonzero column.  Slack columns and guard rows of the input hold 32768 (ruinous if read as data);
    the output buffer starts as a canary (bf16 bits 0x7FC1) and has guard rows before and after and guard columns.
  * Rows of no live query keep the canary: the rows past ``max_len`` of a longer prompt, the rows after the last prompt.
  * The ladder cases rest on v_exp_f32 returning the exact power of two for a small integer argument: measured on an MI355X,
    it does (every ladder case passes bit for bit; P = 2^1 .. 2^8 and alpha = 2^-1 .. 2^-8 all occur, see the CPU file).

test_worst_row_*: the random-data regime of the per-encoder files, held per ROW instead of over the whole output: the worst
single row's relative error of the HIP output against the fp32 truth may not exceed ``slack`` times the worst single row's
error of the bf16 eager flow plus ``floor``, with as_good_as()'s own slack = 1.25 and floor = 5e-4.
"""
import ctypes

import pytest
import torch

from tests import prefill_attn_ref as R
from tests.gpu_common import BF, DEV

pytestmark = pytest.mark.gpu

CANARY = 0x7FC1                  # a bf16 NaN no kernel produces
GUARD = 32768.0                  # input slack and guard rows: finite, exact in bf16, ruinous if read as data


@pytest.fixture(scope="module")
def lib():
    from yat_amd import lib as l
    return l.load()


def _p(t, elems=0):
    return ctypes.c_void_p(t.data_ptr() + 2 * elems)


def _bits(buf):
    b = buf.view(torch.int16)
    return torch.where(b == -32768, torch.zeros_like(b), b)          # -0 folded onto +0


def layout(spec):
    """(q_off, k_off, v_off, ld, out column, ldo, guard rows before, after)"""
    wq, wk = spec.H * spec.dh, spec.Hkv * spec.dh
    if spec.seed % 2 == 0:
        return 0, wq, wq + wk, wq + 2 * wk, 0, wq, 1, 1
    v_off, q_off = 8, 8 + wk + 16
    k_off = q_off + wq + 8
    return q_off, k_off, v_off, k_off + wk + 24, 8, wq + 8 + 16, 2, 3


def run_case(lib, spec):
    c, ref, written = R.case(spec)
    wq, wk, rows = spec.H * spec.dh, spec.Hkv * spec.dh, c["rows"]
    q_off, k_off, v_off, ld, c0, ldo, g0, g1 = layout(spec)
    buf = torch.full((g0 + rows + g1, ld), GUARD, dtype=BF)
    for name, o, w in (("q", q_off, wq), ("k", k_off, wk), ("v", v_off, wk)):
        buf[g0:g0 + rows, o:o + w] = c[name].to(BF)
    buf = buf.to(DEV)
    want = torch.full((g0 + rows + g1, ldo), CANARY, dtype=torch.int16).view(BF)
    want[g0:g0 + rows, c0:c0 + wq][written] = R.expectation(ref[written])
    out = torch.full((g0 + rows + g1, ldo), CANARY, dtype=torch.int16, device=DEV).view(BF)
    off = torch.tensor(c["off"], dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, base, obase = len(spec.lens), g0 * ld, g0 * ldo + c0
    if spec.kind == "vae":
        rc = lib.yat_vae_attn_fwd(B, spec.lens[0], spec.dh, _p(buf, base + q_off), _p(buf, base + k_off), _p(buf, base + v_off),
                                  ld, _p(out, obase), ldo, st)
    elif spec.kind == "gemma":
        rc = lib.yat_gemma_attn_fwd(B, rows, spec.H, spec.Hkv, spec.dh, spec.max_len, R.scale_of(spec), spec.cap, _p(buf, base),
                                    ld, q_off, k_off, v_off, _p(off), _p(out, obase), ldo, st)
    elif spec.kind == "t5":
        table = c["table"].to(BF).to(DEV)
        rc = lib.yat_t5_attn_fwd(B, rows, spec.H, spec.dh, spec.max_len, _p(buf, base), ld, q_off, k_off, v_off, _p(table),
                                 _p(off), _p(out, obase), ldo, st)
    else:
        rc = lib.yat_clip_attn_fwd(B, rows, spec.H, spec.dh, spec.max_len, _p(buf, base), ld, q_off, k_off, v_off,
                                   R.scale_of(spec), _p(off), _p(out, obase), ldo, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return _bits(out).cpu(), _bits(want), (g0, c0)


@pytest.mark.parametrize("spec", R.CASES, ids=R.case_id)
def test_prefill_attn_exact(lib, spec):
    got, want, (g0, c0) = run_case(lib, spec)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, col = bad[0].tolist()
        rows_bad = sorted({int(x) - g0 for x in bad[:, 0].tolist()})
        raise AssertionError(
            f"{bad.shape[0]} elements in {len(rows_bad)} rows differ (rows of the packed matrix: {rows_bad[:12]}...), first at "
            f"(row {r - g0}, column {col - c0}): bits {got[r, col].item() & 0xffff:#06x}, expected "
            f"{want[r, col].item() & 0xffff:#06x}; offsets {c_off(spec)}")


def c_off(spec):
    lens = list(spec.lens)
    return [sum(lens[:i]) for i in range(len(lens) + 1)]


# ---------------------------------------------------------------------------------------------- the per-row bar
SLACK, FLOOR = 1.25, 5e-4                        # as_good_as()'s own (tests/gpu_common.py)


def _row_err(a, truth):
    a, truth = a.float(), truth.float()
    return ((a - truth).norm(dim=-1) / truth.norm(dim=-1).clamp_min(1e-20)).max().item()


def _worst_row(name, hip, flow, truth):
    eh, ef = _row_err(hip, truth), _row_err(flow, truth)
    print(f"[row parity] {name}: worst row hip_vs_fp32={eh:.3e} torchbf16_vs_fp32={ef:.3e}")
    assert torch.isfinite(hip.float()).all()
    assert eh <= SLACK * ef + FLOOR, f"{name}: worst row {eh:.3e} > {SLACK} * the bf16 flow's worst row {ef:.3e} + {FLOOR}"


def test_worst_row_gemma():
    from tests import test_gemma2_gpu as T
    lens, Hq, Hkv = [65, 300, 17], 8, 4
    qkv = T._attn_data(lens, Hq, Hkv, seed=21)
    for cap in (50.0, 0.0):
        _worst_row(f"gemma cap={cap}", T._attn_hip(qkv, lens, Hq, Hkv, cap), T._attn_ref(qkv, lens, Hq, Hkv, cap, BF),
                   T._attn_ref(qkv, lens, Hq, Hkv, cap, torch.float32))


def test_worst_row_t5():
    from tests import test_t5_gpu as T
    lens, H = [65, 300, 17], 3
    qkv = T._attn_data(lens, H, seed=22)
    table = T._table(H, 300, seed=H)
    _worst_row("t5", T._attn_hip(qkv, lens, H, table), T._attn_ref(qkv, lens, H, table, 300, BF),
               T._attn_ref(qkv, lens, H, table, 300, torch.float32))


def test_worst_row_clip():
    from tests import test_clip_gpu as T
    lens, H = [65, 300, 17], 3
    for scale, gain in ((T.DH ** -0.5, 1.0), (1.0, 2.5)):
        qkv = T._attn_data(lens, H, seed=23, gain=gain)
        _worst_row(f"clip scale={scale:g}", T._attn_hip(qkv, lens, H, scale), T._attn_ref(qkv, lens, H, scale, BF),
                   T._attn_ref(qkv, lens, H, scale, torch.float32))


@pytest.mark.parametrize("dh", [64, 512])
def test_worst_row_vae(dh):
    """the data of test_vae_kl_gpu.py::test_attention_against_fp32 at N = 300"""
    import torch.nn.functional as F
    from yat_amd import ops
    N = 300
    g = torch.Generator().manual_seed(dh + N)
    qkv = torch.randn(N, 3 * dh, generator=g)
    qkv[:, :dh] *= 2.0
    qkv[:, 2 * dh:] += 0.5
    qd = qkv.to(BF).to(DEV)
    q, k, v = qd[:, :dh], qd[:, dh:2 * dh], qd[:, 2 * dh:]
    truth = F.scaled_dot_product_attention(q.float()[None, None], k.float()[None, None], v.float()[None, None])[0, 0]
    flow = F.scaled_dot_product_attention(q[None, None], k[None, None], v[None, None])[0, 0]
    out = torch.empty(N, dh, dtype=BF, device=DEV)
    ops.vae_attn_fwd(q, k, v, out, 1, N, dh, 3 * dh, dh)
    _worst_row(f"vae dh={dh}", out, flow, truth)
