"""The conditions test_linear_attn_gpu.py holds the linear-attention kernels to can be met by design, and they bite -- CPU.

tests/linear_attn_ref.py's emulate() is the arithmetic csrc/linear_attn.hip's header describes (fp32 sums of exact products,
a bf16 hi + lo split of S, dU and dS), in torch.  With both halves it stays inside every condition of the GPU file, per
head; with every lo half dropped it stays inside the norm-based ones (bf16 output rounding, 1.65e-3 relative L2, hides the
loss) and breaks the flip cap on every tensor.  So a kernel that fails the cap where this file passes does not compute
what its header says.  Nothing here touches yat_amd.
"""
import pytest
import torch

from tests import linear_attn_ref as R
from tests.gpu_common import _FAILS, _collect_failures, rel  # noqa: F401  (autouse fixture)

NS = (17, 257, 1020, 4096)
B, H = 2, 3
NAMES = ("out", "dq", "dk", "dv")


def _emulate(c, lo):
    D = 32 * c["H"]
    return dict(zip(NAMES, R.emulate(c["qkv"], c["dout"], c["B"], c["N"], c["H"], D, 2 * D, lo=lo)))


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", ("randn", "sparse", "zeros"))
def test_emulation_meets_the_gpu_conditions_and_hi_only_does_not(kind, N):
    c = R.case(kind, B, N, H)
    R.conditions(_emulate(c, True), c, f"emulation {kind} N={N}")
    assert not _FAILS, "; ".join(_FAILS)
    hi_only = _emulate(c, False)
    live = [h for h in range(H) if h not in R.DEAD_HEADS.get(kind, ())]
    for n in NAMES:
        for h in live:
            cols = slice(32 * h, 32 * h + 32)
            nf, numel = R.flips(hi_only[n][:, cols], c["truth"][n][:, cols]), B * N * 32
            print(f"[flips] hi only {kind} N={N} {n} head {h}: {nf} of {numel} = {100 * nf / numel:.2f} %")
            assert nf > R.FLIP_CAP * numel + R.FLIP_FREE, (n, h, nf)


@pytest.mark.parametrize("kind", ("randn", "sparse"))
def test_emulation_at_one_token(kind):
    """N = 1: dq and dk are 0 in exact arithmetic (linear_attn_ref.conditions); the emulation leaves less than 2^-15 of the
    cancelling terms, hi only does not."""
    c = R.case(kind, B, 1, H)
    R.conditions(_emulate(c, True), c, f"emulation {kind} N=1")
    assert not _FAILS, "; ".join(_FAILS)
    R.conditions(_emulate(c, False), c, f"hi only {kind} N=1")
    assert any(" dq head 2" in f for f in _FAILS) and any(" dk head 2" in f for f in _FAILS), _FAILS
    _FAILS.clear()


@pytest.mark.parametrize("N", NS)
def test_emulation_offset_is_as_good_as_the_flow(N):
    """`offset` cancels in dq: no flip cap, but the emulation stays as close to the truth as the flow does, per head."""
    c = R.case("offset", B, N, H)
    got = _emulate(c, True)
    R.conditions(got, c, f"emulation offset N={N}", flip_cap=False)
    mine, flow = R.flip_rates(got, c), R.flip_rates(c["flow"], c)
    for n in NAMES:
        print(f"[flips] offset N={N} {n}: emulation {100 * mine[n]:.2f} %  flow {100 * flow[n]:.2f} %  rel l2 emulation "
              f"{rel(got[n], c['truth'][n]):.3e} flow {rel(c['flow'][n], c['truth'][n]):.3e}")


@pytest.mark.parametrize("N", (1, 17, 257))
def test_truth_is_zero_on_dead_heads(N):
    """`sparse`: head 0 has no live key, head 1 no live query; the fp64 truth of out, dq, dk, dv is exactly 0 there, and
    heads >= 2 are live."""
    c = R.case("sparse", B, N, H)
    for n in NAMES:
        t = c["truth"][n]
        assert torch.isfinite(t).all(), n
        assert not t[:, :64].any(), n
    assert c["truth"]["out"][:, 64:].any() and c["truth"]["dv"][:, 64:].any()


def test_flips_and_rounding():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40, 0.0, -0.0, 3.0], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -7, 1.0, 0.0, 0.0, 3.0]).to(torch.bfloat16)      # a tie in fp32, not in fp64
    assert torch.equal(R.round_bf16(t), want)
    assert R.flips(want, t) == 0
    assert R.flips(torch.tensor([1.0, 1.0, 1.0, -0.0, 0.0, 3.0]).to(torch.bfloat16), t) == 1
    assert R.flips(torch.tensor([1.0, 1.0, 1.0, -0.0, 0.0, float("nan")]).to(torch.bfloat16), t) == 2


@pytest.mark.parametrize("kind", R.KINDS)
def test_inputs_are_what_they_say(kind):
    qkv, dout = R.make_inputs(kind, 2, 40, 4)
    x = qkv.float().view(2, 40, 3, 4, 32)
    assert torch.isfinite(x).all() and not ((x != 0) & (x.abs() < 2.0 ** -126)).any()
    q, k = x[:, :, 0], x[:, :, 1]
    if kind == "sparse":
        assert not (k[:, :, 0] > 0).any() and not (q[:, :, 1] > 0).any()
        assert not (q[:, 3::7] > 0).any() and not (k[:, 3::5] > 0).any()
        assert (q[:, :, 2:] > 0).flatten(1).any(1).all() and (k[:, :, 2:] > 0).flatten(1).any(1).all()
    if kind == "zeros":
        neg = (qkv.view(torch.int16) == -32768).float().mean().item()
        pos = ((qkv == 0).float().mean().item()) - neg
        assert 0.08 < neg < 0.12 and 0.08 < pos < 0.12


def test_reference_takes_strided_inputs():
    Bq, N, Hq = 2, 19, 3
    D = 32 * Hq
    qkv, dout = R.make_inputs("randn", Bq, N, Hq)
    wide = torch.full((Bq * N + 5, 3 * D + 24), float("nan"), dtype=torch.float64)
    view = wide[5:]
    view[:, :D], view[:, D:2 * D], view[:, 2 * D + 8:3 * D + 8] = qkv[:, :D], qkv[:, 2 * D:], qkv[:, D:2 * D]
    a = R.reference(view, Bq, N, Hq, 2 * D + 8, D, torch.float64)
    b = R.reference(qkv, Bq, N, Hq, D, 2 * D, torch.float64)
    assert torch.equal(a, b)
