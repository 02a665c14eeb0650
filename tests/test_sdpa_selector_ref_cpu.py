"""The selector inputs of tests/sdpa_selector_ref.py are what test_sdpa_exact_gpu.py takes them for -- CPU.

For every case of the GPU file's parameter lists (imported, not copied), on the plain fp64 reference:
  * the softmax weights are exactly 1, 1/2 or 1/4, or below 2^-150; the row maximum is +256 or -64 (powers of two: the
    winners' exponentials are exactly 1 in the kernels' fp32) and every other score is at least 128 lower;
  * dS fits bf16, is a multiple of 1/16 and at most 4, |dP - delta| <= 16 where P > 0;
  * out and out_dense fit bf16, delta fp32; dq, dk, dv (ROUNDED_ONCE) fit fp32; every sum of magnitudes stays below 2^24
    in units of its smallest step, so an fp32 accumulation in any order is exact;
  * in every (image, head) some query selects the last live key, and the key just past the limit is a masked duplicate
    that would tie a winner without its bias (kv_len < T) or the zero-filled phantom (kv_len = T).
"Fits" allows 2^-140 absolute: the weights below 2^-150 leave that much in the fp64 sums and nothing in the fp32 ones.
Over the list: every column of every head dim carries a nonzero expectation in out, out_dense, dq, dk and dv; the lists reach every
instantiation the host can select (the restated dispatch, sdpa_selector_ref.dispatch) and both xcd_remap states.
"""
import pytest
import torch

from tests import sdpa_selector_ref as R

TINY = 2.0 ** -140
_COLS = {}           # case -> {tensor name: [dh] bool, columns with a nonzero expectation in some row of some head}


def _fits(x, dtype):
    return bool(((x.to(dtype).double() - x).abs() <= TINY).all())


def _columns(spec, exp):
    H, dh = spec[3], spec[4]
    _COLS[spec] = {n: (exp[n].float().view(-1, H, dh) != 0).any(0).any(0) for n in ("out", "out_dense", "dq", "dk", "dv")}


@pytest.mark.parametrize("spec", R.CASES, ids=R.case_id)
def test_case_is_exact_by_construction(spec):
    B, N, T, H, dh, lens, seed, scale, sign = spec
    c = R.build(B, N, T, H, dh, None if lens is None else list(lens), seed, scale, sign)
    r = R.reference(c, weights=True)
    p, ds, s = r["p"], r["ds"], r["s"]
    top = s.max(-1, keepdim=True).values
    assert bool((top == (256.0 if sign > 0 else -64.0)).all())
    assert bool(((s == top) | (s <= top - 128)).all())
    assert bool(((p == 1) | (p == 0.5) | (p == 0.25) | (p < 2.0 ** -150)).all())
    assert bool(((p > 0.2) == (s == top)).all())
    q, dout = (c[n].double().view(B, N, H, dh).transpose(1, 2) for n in ("q", "dout"))
    k, v = (c[n].double().view(B, T, H, dh).transpose(1, 2) for n in ("k", "v"))
    # bf16 intermediates and the integer bounds
    dpd = dout @ v.transpose(-1, -2) - r["delta"][..., None]
    assert float((dpd.abs() * (p > 0.2)).max()) <= 16
    assert _fits(ds, R.BF) and float(ds.abs().max()) <= 4
    assert bool((((ds * 16).round() - ds * 16).abs() <= TINY).all())
    assert float((q.abs() @ k.abs().transpose(-1, -2)).max()) < 2 ** 24                    # scores, unit 1
    assert float((p @ v.abs()).max()) * 4 < 2 ** 24                                          # out, unit 1/4
    assert float((ds.abs() @ k.abs()).max()) * 16 < 2 ** 24                                  # dq / scale, unit 1/16
    assert float((ds.abs().transpose(-1, -2) @ q.abs()).max()) * 16 < 2 ** 24                # dk / scale, unit 1/16
    assert float((p.transpose(-1, -2) @ dout.abs()).max()) * 4 < 2 ** 24                     # dv, unit 1/4
    assert _fits(r["out"], R.BF) and _fits(r["out_dense"], R.BF) and _fits(r["delta"], torch.float32)
    assert float(r["out_dense"].abs().max()) <= 8
    for n in R.ROUNDED_ONCE:
        assert _fits(r[n], torch.float32), n
    # the edge of every image: the last live key is selected, the next one would be were it not masked
    for b, L in enumerate(c["live"]):
        assert bool((p[b, :, :, L - 1] > 0.2).any(-1).all()), (b, L)
        if L < T:
            unbiased = s[b, :, :, L] - float(c["key_bias"][b, L])
            assert float(c["key_bias"][b, L]) == R.MODEL_BIAS and bool((unbiased == top[b, :, :, 0]).any(-1).all()), (b, L)
            assert bool((p[b, :, :, L:] == 0).all())
    exp = R.expectation(r)
    g = torch.round(1 / p.max(-1).values)
    assert bool((exp["one_winner"] == (g == 1)).all())
    assert bool(((r["lse"] - (top[..., 0] + torch.log(g))).abs() < 1e-12).all())
    _columns(spec, exp)


def test_every_column_carries_a_nonzero_expectation():
    for spec in R.CASES:
        if spec not in _COLS:                      # (run on its own)
            _columns(spec, R.case(spec)[2])
    for dh in sorted({s[4] for s in R.CASES}):
        for n in ("out", "out_dense", "dq", "dk", "dv"):
            seen = torch.zeros(dh, dtype=torch.bool)
            for spec, cols in _COLS.items():
                if spec[4] == dh:
                    seen |= cols[n]
            assert bool(seen.all()), (dh, n, (~seen).nonzero().flatten().tolist())


def test_lists_reach_every_host_reachable_instantiation():
    fwd, dq, dkv, xcd, xcd_dkv = set(), set(), set(), set(), set()
    work_heads = []
    for B, N, T, H, dh, lens, *_ in R.CASES:
        d = R.dispatch(B, N, T, H, dh, lens is not None)
        fwd.add(d["fwd"]); dq.add(d["dq"]); dkv.add(d["dkv"])
        xcd.add((d["fwd"][3], d["xcd"])); xcd_dkv.add((d["dkv"][3], False, d["xcd_dkv"]))
        if lens is not None:                       # the GPU file runs every bias case again with a work list
            w = R.dispatch(B, N, T, H, dh, True, work=True)
            dkv.add(w["dkv"]); xcd_dkv.add((False, True, w["xcd_dkv"]))
            assert w["dkv"][2] == 1 and w["xcd_dkv"]
            work_heads.append(sum(-(-(L if L > 0 else T) // 64) for L in lens) * H)
    assert fwd == R.REACHABLE_FWD, (R.REACHABLE_FWD - fwd, fwd - R.REACHABLE_FWD)
    assert dq == R.REACHABLE_DQ, (R.REACHABLE_DQ - dq, dq - R.REACHABLE_DQ)
    assert dkv == R.REACHABLE_DKV, (R.REACHABLE_DKV - dkv, dkv - R.REACHABLE_DKV)
    # xcd_remap on and off, with and without a bias (forward / dQ), dense with and without a bias and the work list (dK/dV)
    assert xcd == {(nb, x) for nb in (False, True) for x in (False, True)}
    assert xcd_dkv >= {(False, False, False), (False, False, True), (True, False, False), (True, False, True), (False, True, True)}
    assert any(w % 8 for w in work_heads)          # work-list grids that are no multiple of the 8 XCDs
    x = [c for c in R.XCD if c[5] is not None][0]
    assert (sum(-(-(L if L > 0 else x[2]) // 64) for L in x[5]) * x[3]) % 8


def test_dispatch_restatement_at_known_shapes():
    """shapes whose classes the kernel file's comments and the earlier tests name"""
    assert R.dispatch(2, 90, 90, 2, 104, False)["fwd"] == (4, 7, 1, True, False)           # 104 is no ONES head dim
    assert R.dispatch(8, 130, 130, 64, 112, False)["fwd"] == (4, 8, 2, True, True)
    assert R.dispatch(8, 258, 65, 64, 32, False)["fwd"] == (1, 3, 4, True, True)
    assert R.dispatch(8, 258, 65, 64, 40, False)["fwd"] == (2, 4, 2, True, False)           # wide = 3 without a ONES class
    assert R.dispatch(8, 200, 65, 64, 72, True)["fwd"] == (3, 5, 3, False, False)
    assert R.dispatch(8, 200, 65, 64, 72, True)["dq"] == (3, 5, 2, False)
    assert R.dispatch(8, 200, 65, 64, 64, True)["dq"] == (2, 4, 3, False)
    assert R.dispatch(8, 17, 130, 64, 80, True)["dkv"] == (3, 5, 2, False)
    assert R.dispatch(8, 17, 130, 64, 88, True)["dkv"] == (4, 7, 1, False)
    assert R.dispatch(1, 1030, 1030, 1, 64, False)["xcd"] and not R.dispatch(1, 64, 1023, 1, 64, False)["xcd"]


def test_narrow_lists_hold_the_sizes_the_kernels_branch_on():
    bias = [c for c in R.NARROW if c[5] is not None]
    assert {c[1] for c in R.NARROW} == set(R.NS) and {c[2] for c in R.NARROW} == set(R.TS)
    assert {c[4] for c in bias} == set(R.DH_BIAS) and {c[4] for c in R.NARROW if c[5] is None} == set(R.DH_NOBIAS)
    assert {(c[0], c[3]) for c in R.NARROW} >= {(3, 3), (1, 3), (3, 1)}
    kinds = set()
    for c in bias:
        T = c[2]
        for L in c[5]:
            kinds |= {n for n, val in (("all", 0), ("1", 1), ("63", 63), ("64", 64), ("65", 65), ("T-1", T - 1), ("T", T)) if L == val}
    assert kinds == {"all", "1", "63", "64", "65", "T-1", "T"}
    for sign in (1, -1):                                     # both sign variants at every head dim, with and without a bias
        assert {c[4] for c in bias if c[8] == sign} == set(R.DH_BIAS)
        assert {c[4] for c in R.NARROW if c[5] is None and c[8] == sign} == set(R.DH_NOBIAS)
