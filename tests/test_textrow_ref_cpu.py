"""The properties test_textrow_exact_gpu.py rests on, proven on the CPU from tests/textrow_ref.py, and the argument checks
of the ops wrappers that take a pointer and a row stride."""
import numpy as np
import pytest
import torch

from tests import textrow_ref as R


def test_widths_reach_every_lanes_per_row_class():
    low = {(D >> 3) & -(D >> 3) for D in R.NORM_D}                      # lowest set bit of D / 8
    assert low == {1, 2, 4, 8, 16, 32, 64, 128}
    assert {R.lpr_of(D) for D in R.NORM_D} == {1, 2, 4, 8, 16, 32, 64}
    assert min(R.NORM_D) == 8 and R.chunk_passes(8) == 1
    assert any(R.lpr_of(D) == 64 and R.chunk_passes(D) == 1 for D in R.NORM_D)         # 512
    assert any(R.lpr_of(D) == 64 and R.chunk_passes(D) > 1 for D in R.NORM_D)          # 1024 (capped), 1536
    assert any(R.lpr_of(D) == 1 and R.chunk_passes(D) > 1 for D in R.NORM_D)           # 24
    for D in R.NORM_D:
        rpb = 256 // R.lpr_of(D)
        assert {1, rpb, rpb + 1, 2 * rpb + 1} <= set(R.norm_rows(D)) and (rpb == 1 or rpb - 1 in R.norm_rows(D))
        assert all(D % 8 == 0 and D % 4 == 0 for D in R.NORM_D)


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("D", R.NORM_D)
def test_rows_are_exact(D, centered):
    for family, ms in (("pow4", 1.0), ("five", 25.0)):
        M = R.norm_rows(D)[-1]
        s, mu, k = R.rows(M, D, family, seed=D, centered=centered)
        R.to_bf(s)                                                       # exact in bf16
        if centered:
            assert np.array_equal(s.sum(-1, keepdims=True), mu * D) and (mu != 0).any()      # the mean is mu, from an integer sum
        d = s - mu
        ss = (d ** 2).sum(-1, keepdims=True)
        # every square is an integer and the whole sum stays below 2^24: fp32 accumulation is exact in any order
        assert np.array_equal(d, np.round(d)) and ss.max() < 2 ** 24
        assert np.array_equal(ss / D, ms * 4.0 ** k)                     # the mean square: a power of 4 (times 25)
        rs = R.rstd(s, mu)
        if family == "pow4":
            assert np.array_equal(rs, (2.0 ** -k).astype(np.float32))    # an exact power of two
            assert np.array_equal(np.abs(d * rs), np.ones_like(d))
        else:
            assert np.array_equal(rs, (np.float32(1.0) / np.float32(5.0)) * (2.0 ** -k).astype(np.float32))
            v = (d.astype(np.float32) * rs).astype(np.float32)
            assert (R.rbf(v) != v).any()                                 # x rs is not a bf16 number: the roundings can be told apart


@pytest.mark.parametrize("D", R.NORM_D)
def test_pow4_expectations_are_rounded_once_and_off_every_tie(D):
    M = R.norm_rows(D)[-1]
    s, _, _ = R.rows(M, D, "pow4", seed=D + M)
    w = R.weights(D, D, fine=True)
    t = R.expected_gemma(s, w).astype(np.float64)
    assert np.array_equal(np.abs(t), np.abs(1.0 + w) * np.ones_like(s)) and not R.on_tie(t).any()
    assert (R.rbf(t) != t).any()                                         # 11 significant bits: the store does round
    res = R.coarse((M, D), D + M) * 8
    res = np.where(R.on_tie(R.expected_gemma(s, w, res).astype(np.float64)), 0.0, res)
    assert not R.on_tie(R.expected_gemma(s, w, res).astype(np.float64)).any() and (res != 0).mean() > 0.7
    w5 = R.weights(D, D + 1)
    assert np.array_equal(np.abs(R.expected_t5(s, w5)), np.abs(w5) * np.ones_like(s))      # exact: no rounding at all
    sc, mu, _ = R.rows(M, D, "pow4", seed=5 * D + M, centered=True)
    ln = R.expected_layernorm(sc, mu, R.coarse(D, D + 2), R.coarse(D, D + 3)).astype(np.float64)
    assert np.array_equal(R.rbf(ln), ln)                                 # multiples of 1/32 below 8: exact in bf16
    dc = R.expected_dcae(s, R.coarse(D, D), R.coarse(D, D + 1), R.coarse((M, D), D + M))
    assert np.array_equal(np.abs(dc) * 32, np.round(np.abs(dc) * 32)) and np.abs(dc).max() <= 6


def test_five_family_tells_the_roundings_apart():
    s, _, _ = R.rows(9, 96, "five", seed=1)
    w = R.weights(96, 2)
    two, one = R.rbf(R.expected_t5(s, w)), R.rbf(R.expected_t5_one_rounding(s, w))
    assert (two != one).any()


def test_on_tie():
    assert R.on_tie(np.array([1.00390625]))[0] and not R.on_tie(np.array([1.0078125, 1.005859375, 3.0, 0.0])).any()


def test_rope_inputs_are_exact_and_tell_a_swap():
    for dh, heads, vheads, slack, lens in R.ROPE_CASES:
        x, pos, cos, sin, ld = R.rope_case(dh, heads, vheads, slack, lens)
        assert ld > heads * dh and ld % 8 == 0 and (x.shape[0] * heads * (dh // 16)) % 256 != 0
        assert list(pos[:lens[0]]) == list(range(lens[0])) and (len(lens) == 1 or pos[lens[0]] == 0)
        want = R.rope_ref(x, pos, cos, sin, heads, dh)
        R.to_bf(want)
        # each product is exact in bf16 on its own (the module rounds both), and a sign or half swap changes values
        R.to_bf(x[:, :heads * dh] * np.tile(cos[pos], heads))
        assert not np.array_equal(want, R.rope_ref(x, pos, cos, -sin, heads, dh))
        assert np.array_equal(want[:, heads * dh:], x[:, heads * dh:])
    assert {c[0] for c in R.ROPE_CASES} == {16, 64, 256}


def test_geglu_and_embed_case_shapes():
    assert any((M * N // 8) % 256 for M, N, _, _ in R.GEGLU_CASES) and any(M * N // 8 > 256 for M, N, _, _ in R.GEGLU_CASES)
    assert any(D == 8 for _, D, _ in R.EMBED_CASES) and any(D % 64 for _, D, _ in R.EMBED_CASES if D > 8)
    for n, D, vocab in R.EMBED_CASES:
        c = R.embed_case(n, D, vocab, npos=vocab + 2)
        assert (n * D // 8) % 256 != 0 and 0 in c["ids"].tolist() + c["pos"].tolist()
        assert n == 1 or (vocab - 1 in c["ids"].tolist() and vocab + 1 in c["pos"].tolist())


def test_wrappers_refuse_a_strided_last_dimension():
    """A view whose columns are not adjacent cannot be described by pointer + ld: ValueError before any library call (no
    library is loaded here: the check comes first)."""
    from yat_amd import ops
    bf = torch.bfloat16
    wide = torch.zeros(4, 64, dtype=bf)
    strided, ok = wide[:, ::2], torch.zeros(4, 32, dtype=bf)
    off = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="contiguous last dimension"):
        ops.gemma_attn_fwd(strided, off, 1, 1, 1, 256, 4, 1.0, 0.0, ok)
    with pytest.raises(ValueError, match="contiguous last dimension"):
        ops.gemma_attn_fwd(ok, off, 1, 1, 1, 256, 4, 1.0, 0.0, strided)
    with pytest.raises(ValueError, match="contiguous last dimension"):
        ops.t5_attn_fwd(ok, off, 1, 1, 64, 4, torch.zeros(1, 7, dtype=bf), strided)
    with pytest.raises(ValueError, match="contiguous last dimension"):
        ops.clip_attn_fwd(strided, off, 1, 1, 64, 4, 1.0, ok)
    with pytest.raises(ValueError, match="contiguous last dimension"):
        ops.vae_attn_fwd(ok, ok, ok, strided, 1, 4, 64, 32)
    with pytest.raises(ValueError, match="contiguous last dimension"):
        ops.geglu(ok, 16, strided)
    with pytest.raises(ValueError, match="contiguous last dimension"):
        ops.rope_qk(strided, 1, 16, torch.zeros(4, dtype=torch.int32), torch.zeros(4, 16, dtype=bf), torch.zeros(4, 16, dtype=bf))
