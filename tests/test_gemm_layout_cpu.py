"""The case table of test_gemm_layout_gpu.py reaches every class it is meant to, and its checker bites -- CPU.

tests/gemm_ref.py holds the table, the fp32 model and check().  Here a plain-torch executor that addresses memory the way the
kernels do (base pointer + leading dimension) stands in for the GPU: the correct one passes check() and close(window, model)
on every case; with one planted error each (gemm_ref.FAULTS) at least one case of the table reports it.  Errors of placement --
a store past N or M, a wrong leading dimension, a read past an operand's width -- are reported by check() alone.  The two
errors of arithmetic (the ragged last K chunk dropped, the gate row taken from m / M) are made by the contiguous launch as well,
so check() cannot see them: close(window, model), the other condition of the GPU file, does.  Nothing here touches yat_amd.
"""
import collections

import pytest
import torch

from tests import gemm_ref as R
from tests.gpu_common import _FAILS, _collect_failures, close  # noqa: F401  (autouse fixture)


def _run(case, fault=None):
    """-> (failures of check(), failures of close(window, model)) of the CPU executor on one case"""
    before, twin = R.build(case, seed=1)
    after = R.clone(before)
    R.cpu_execute(case, R.views(case, after), fault)
    tv = R.twin_views(case, R.clone(twin))
    R.cpu_execute(case, tv, fault)
    fails = R.check(case, before, after, tv)
    v = R.views(case, after)
    want = R.model(case, R.views(case, before), own=v.get("aux"))
    for name, ref in want.items():
        if name == "rowsum":
            close(v[name], ref, f"{case.name} {name}", tol=4e-3, ulps=3.0)
        else:
            close(v[name], ref, f"{case.name} {name}")
    parity = list(_FAILS)
    _FAILS.clear()
    return fails, parity


@pytest.fixture(scope="module")
def correct():
    return {c.name: _run(c) for c in R.TABLE}


def test_correct_executor_passes_every_case(correct):
    bad = {n: f for n, f in correct.items() if f[0] or f[1]}
    assert not bad, bad


def test_table_reaches_every_class(capsys):
    cl = [R.classes(c) for c in R.TABLE]
    count = collections.Counter()
    for c, k in zip(R.TABLE, cl):
        for key in ("group", "placement", "epi", "layout", "path"):
            count[f"{key}={k[key]}"] += 1
        count[f"group={k['group']} placement={k['placement']}"] += 1
        count["wide" if k["wide"] else "narrow"] += 1
        count[f"{'wide' if k['wide'] else 'narrow'} tile={c.tile}"] += 1
        for flag in ("ragged_m", "ragged_n", "ragged_k", "n_mod8_is_4"):
            count[flag] += k[flag]
        for name in k["ld4"]:
            count[f"ld4={name}"] += 1
        count[f"tiles(v{c.tile})={k['tiles'].get(c.tile, k['tiles'][1])}"] += 1
        if c.res == "out":
            count[f"accumulate {k['layout']}"] += 1
    with capsys.disabled():
        print(f"\n[gemm layout] {len(R.TABLE)} cases")
        for key in sorted(count):
            print(f"[gemm layout] {key}: {count[key]}")
    need = [f"group={g} placement={p}" for g in ("wide", "narrow_n", "narrow_ld", "rank") for p in ("a", "b", "c", "abc", "mid")]
    need += [f"epi={e}" for e in R.EPIS] + [f"layout={x}" for x in R.LAYOUTS] + [f"path={p}" for p in (0, 1, 4, 5, 204, 305)]
    need += [f"ld4={m}" for m in ("c", "aux", "res", "gate", "pre", "dact")]
    need += ["narrow tile=1", "narrow tile=4", "narrow tile=5", "wide tile=4", "wide tile=5", "ragged_m", "ragged_n", "ragged_k",
             "n_mod8_is_4", "accumulate TN", "accumulate NN", "tiles(v4)=(2, 2)", "tiles(v5)=(2, 2)", "tiles(v1)=(3, 3)"]
    assert not [n for n in need if not count[n]]
    # narrow by N: every tile variant ends its last column tile on a 4-column group at N = 332
    assert {(c.tile, c.layout) for c in R.TABLE if c.N == 332} >= {(v, x) for v in (1, 4, 5) for x in ("NT", "TT")}
    # the chain in every narrow class and on both split-K paths; glu_u wide only; a_rowsum with a strided A
    assert {c.group for c in R.TABLE if c.epi == "chain"} >= {"wide", "narrow_n", "narrow_ld"}
    assert {c.path for c in R.TABLE if c.epi == "chain"} >= {1, 4, 5, 204, 305}
    assert all(R.wide(c) and c.c.ld > 2 * c.N for c in R.TABLE if c.glu)
    assert all(c.a.ld > c.M and c.layout == "TN" and c.path in (0, 4) for c in R.TABLE if c.rowsum)
    assert all(R.wide(c) for c in R.TABLE if c.path > 100)


def test_narrow_by_stride_flips_the_predicate_on_its_own():
    cases = [c for c in R.TABLE if c.group == "narrow_ld"]
    assert {(c.member, c.tile) for c in cases} >= {(m, v) for m in ("c", "aux", "res", "gate", "pre", "dact") for v in (4, 5)}
    assert {c.layout for c in cases if c.member in ("c", "aux", "res", "gate")} == set(R.LAYOUTS)
    for c in cases:
        ld = R.lds(c)
        assert c.N % 8 == 0 and R.classes(c)["ld4"] == (c.member,) and not R.wide(c), c.name
        assert all(v % 8 == 0 for k, v in ld.items() if k != c.member), c.name
        assert R.wide(c, {**ld, c.member: ld[c.member] + 4}), c.name
        assert c.c.col == 4 + (c.N if c.placement == "mid" else 0) and (c.aux is None or c.aux.col == 4), c.name


def test_dimensions_and_alignment():
    for c in R.TABLE:
        assert max(c.M, c.N) < R.MAX_DIM and (c.K < R.MAX_DIM or c.K == R.SPLIT_K), c.name
        assert (c.path > 100) == (c.K == R.SPLIT_K), c.name
        # what the entry point requires: 16-byte chunks of A and B, 8-byte groups of C; 16-byte epilogue accesses when wide
        assert c.a.col % 8 == 0 and c.b.col % 8 == 0 and c.a.ld % 8 == 0 and c.b.ld % 8 == 0, c.name
        step = 8 if R.wide(c) else 4
        for name, (rows, cols, p) in R.shapes(c).items():
            assert p.col + cols <= p.ld, (c.name, name)
            if name not in ("a", "b"):
                assert p.col % step == 0 and p.ld % step == 0, (c.name, name)
        assert c.bias is None or c.bias[0] % step == 0, c.name
        assert c.N % 4 == 0 and (not c.b_t or c.N % 8 == 0) and (not c.a_t or c.M % 8 == 0) and c.K % 8 == 0, c.name


def test_build_pads_with_nan_and_sentinel():
    case = next(c for c in R.TABLE if c.epi == "chain" and c.group == "wide" and c.path == 4)
    bufs, twin = R.build(case, seed=1)
    v = R.views(case, bufs)
    for name, buf in bufs.items():
        inside = R._window_mask(case, name, buf) if name in R.OUTPUTS else None
        if name in R.OUTPUTS:
            assert (R.bits(buf) == R.bits(R._sentinel(1))[0]).all(), name
            assert inside.sum() == v[name].numel()
        else:
            assert torch.isnan(buf.float()).sum() == buf.numel() - v[name].numel(), name
            assert torch.equal(v[name], twin[name]), name
    assert torch.isnan(R._sentinel(1).float()).all() and not (R.bits(torch.tensor([float("nan")], dtype=R.BF)) ==
                                                              R.bits(R._sentinel(1))).any()


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_error_is_caught(fault, correct):
    caught_by_check, caught_by_model = [], []
    for c in R.TABLE:
        fails, parity = _run(c, fault)
        if fails:
            caught_by_check.append(c.name)
        if parity:
            caught_by_model.append(c.name)
        if len(caught_by_check if fault not in R.ARITHMETIC_FAULTS else caught_by_model) >= 3:
            break                                           # (one would do; the table is not walked to its end for a count)
    print(f"[gemm layout] {fault}: check() reports {caught_by_check}, close(window, model) {caught_by_model}")
    if fault in R.ARITHMETIC_FAULTS:
        assert caught_by_model, fault
    else:
        assert caught_by_check, fault
