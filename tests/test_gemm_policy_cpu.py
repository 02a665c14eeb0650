"""The GEMM host policy (yat_amd/csrc/gemm_policy.hpp) is a pure function, so it is pinned here without a GPU: a stand-alone
probe (tests/gemm_policy_probe.cpp) is built with a host compiler and asked every query of the grid below; its picks must
equal, row for row, the picks recorded from the policy as it stood before it became a header
(tests/golden/gemm_policy_picks.json; profiles/gemm_policy_a_picks.txt says how they were recorded).

A query is (a_t, b_t, M, N, K, K2, class, wide_ok, a2_group, workspace MiB, policy word); a pick is -1 (refused) or
tile * 10000 + ksplit * 100 + group.  Only queries whose ARGUMENTS yat_gemm_bf16_ex accepts are in the grid (operand byte
ranges below 2 GiB, N % 8 == 0 where B is k-strided): what is pinned is the policy, not the argument checks."""
import hashlib
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_policy_picks.json")
PROBE_SRC = os.path.join(ROOT, "tests", "gemm_policy_probe.cpp")

MS = (8, 1000, 1024, 8192, 32768)
NS = (32, 252, 256, 320, 512, 1152, 2240, 5600, 11200)            # 252: N % 8 == 4, wide_ok false
KS = (64, 256, 512, 2048, 2240, 8192, 32768)
LAYOUTS = ((0, 0), (0, 1), (1, 1), (1, 0))
STREAMS = (1, 2, 8)
WS_MIB = (0, 1, 96)                                                # 0: no workspace
TILES = (0, 1, 4, 5)
SPLITS = (0, 2, 32, 33)
GROUPS = (0, 8, 65)
A2_GROUPS = (0, 256, 320, 640, 100)
K2S = (64, 96)
PLAIN, GLU_BWD, PRE_ADD, ACT_BWD, ROWSUM, PAIR2 = range(6)
HOME_LAYOUT = {PLAIN: (0, 0), GLU_BWD: (0, 1), PRE_ADD: (0, 0), ACT_BWD: (0, 1), ROWSUM: (1, 1), PAIR2: (0, 0)}
COLS = ("a_t", "b_t", "M", "N", "K", "K2", "cls", "wide", "a2_group", "ws_mib", "word")
LIMIT = 0x7fffffff


def leading_dims(a_t, b_t, M, N, K, K2, cls, a2_group):
    """lda, ldb a caller would pass (the second operand pair's columns share A's and B's rows)."""
    blocks = -(-N // a2_group) if a2_group > 0 else 1
    lda = max(M if a_t else K, blocks * K2 if cls == PAIR2 else 0)
    ldb = max(N if b_t else K, K2 if cls == PAIR2 else 0)
    return (lda + 7) // 8 * 8, (ldb + 7) // 8 * 8


def row(a_t, b_t, M, N, K, cls, wide, ws, tile, split, streams, group, K2=0, a2_group=0):
    """One query, or None where the argument checks in front of the policy refuse the call."""
    if b_t and N % 8:
        return None
    if cls != PAIR2:
        K2 = a2_group = 0
    lda, ldb = leading_dims(a_t, b_t, M, N, K, K2, cls, a2_group)
    blocks = -(-N // a2_group) if a2_group > 0 else 1
    nbytes = [(K if a_t else M) * lda * 2, (K if b_t else N) * ldb * 2]
    if cls == PAIR2:
        nbytes += [((M - 1) * lda + blocks * K2) * 2, ((N - 1) * ldb + K2) * 2]
    if max(nbytes) > LIMIT:
        return None
    wide = int(bool(wide) and N % 8 == 0)
    return (a_t, b_t, M, N, K, K2, cls, wide, a2_group, ws, tile + 100 * split + 10000 * streams + 1000000 * group)


def _lcg(seed):
    x = seed
    while True:
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        yield x >> 33


def _sampled(cls, count, seed):
    """``count`` draws from the whole cross product of one class, forced words and forbidden combinations included."""
    rnd = _lcg(seed)
    pick = lambda seq: seq[next(rnd) % len(seq)]
    for _ in range(count):
        (a_t, b_t) = pick(LAYOUTS) if next(rnd) % 3 == 0 else HOME_LAYOUT[cls]
        yield row(a_t, b_t, pick(MS), pick(NS), pick(KS), cls, next(rnd) % 4 != 0, pick(WS_MIB), pick(TILES), pick(SPLITS),
                  pick(STREAMS), pick(GROUPS), pick(K2S), pick(A2_GROUPS))


def grid():
    rows = []
    # plain class, automatic word: the whole cross product
    for (a_t, b_t), M, N, K, s, ws in itertools.product(LAYOUTS, MS, NS, KS, STREAMS, WS_MIB):
        rows.append(row(a_t, b_t, M, N, K, PLAIN, 1, ws, 0, 0, s, 0))
    # plain class, forced tile
    for (a_t, b_t), M, N, K, tile, ws in itertools.product(LAYOUTS, MS, NS, KS, TILES[1:], (0, 96)):
        rows.append(row(a_t, b_t, M, N, K, PLAIN, 1, ws, tile, 0, 1, 0))
    rows.extend(_sampled(PLAIN, 3000, 1))
    for cls in (GLU_BWD, PRE_ADD, ACT_BWD, ROWSUM, PAIR2):
        a_t, b_t = HOME_LAYOUT[cls]
        for i, (M, N, K, s) in enumerate(itertools.product(MS, NS, KS, STREAMS)):
            rows.append(row(a_t, b_t, M, N, K, cls, 1, 96, 0, 0, s, 0, K2S[0], A2_GROUPS[i % 4]))
        rows.extend(_sampled(cls, 1500, 10 + cls))
    seen, out = set(), []
    for r in rows:
        if r is not None and r not in seen:
            seen.add(r)
            out.append(r)
    return out


def grid_text(rows):
    return "".join(" ".join(map(str, r)) + "\n" for r in rows)


@pytest.fixture(scope="module")
def rows():
    return grid()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def picks(rows, tmp_path_factory):
    """Every query asked twice in ONE run of the probe: the whole grid, then the whole grid again."""
    from yat_amd.build import _hipcc
    exe = str(tmp_path_factory.mktemp("gemm_policy") / "probe")
    hipcc = _hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    cxx = shutil.which("c++") or shutil.which("g++") or (clang if os.path.exists(clang) else None)
    assert cxx, "no host C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", PROBE_SRC, "-o", exe], check=True)
    text = grid_text(rows)
    out = subprocess.run([exe], input=text + text, capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 2 * len(rows)
    return [int(v) for v in out]


def test_grid_is_the_recorded_one(rows, golden):
    assert len(rows) == golden["rows"] == len(golden["picks"])
    assert hashlib.sha1(grid_text(rows).encode()).hexdigest() == golden["grid_sha1"]


def test_grid_covers_every_axis_value_per_class(rows, golden):
    refused = {cls: 0 for cls in range(6)}
    for r, g in zip(rows, golden["picks"]):
        refused[r[6]] += g < 0
    for cls in range(6):
        mine = [r for r in rows if r[6] == cls]
        word = lambda r, div, mod: r[10] // div % mod
        for idx, axis in ((2, MS), (3, NS), (4, KS), (9, WS_MIB)):
            assert {r[idx] for r in mine} >= set(axis), (cls, COLS[idx])
        assert {(r[0], r[1]) for r in mine} == set(LAYOUTS), cls
        assert {word(r, 1, 100) for r in mine} >= set(TILES) and {word(r, 100, 100) for r in mine} >= set(SPLITS), cls
        assert {word(r, 10000, 100) for r in mine} >= set(STREAMS) and {r[10] // 1000000 for r in mine} >= set(GROUPS), cls
        assert {r[7] for r in mine} == {0, 1}, cls
        assert any(word(r, 100, 100) > 1 and word(r, 1, 100) == t for r in mine for t in (0, 1)), cls
        assert refused[cls] >= 2, cls
    pair = [r for r in rows if r[6] == PAIR2]
    assert {r[8] for r in pair} >= set(A2_GROUPS) and {r[5] for r in pair} >= set(K2S)


def test_every_pick_equals_the_recorded_one(rows, picks, golden):
    bad = [(r, got, want) for r, got, want in zip(rows, picks, golden["picks"]) if got != want]
    assert not bad, f"{len(bad)} of {len(rows)} picks differ, first (query {COLS}, got, recorded): {bad[:5]}"


def test_same_query_same_plan(rows, picks):
    """No state from call to call: each query's second answer, given after every other query was asked, is its first."""
    assert picks[:len(rows)] == picks[len(rows):]


def test_plan_properties(rows, picks):
    for r, pick in zip(rows, picks):
        if pick < 0:
            continue
        a_t, b_t, M, N, K, K2, cls, wide, a2_group, ws, word = r
        tile, ksplit, group = pick // 10000, pick // 100 % 100, pick % 100
        assert tile in (1, 4, 5) and 1 <= ksplit <= 32 and group <= 64, r
        if ksplit > 1:
            assert ws > 0 and ksplit * M * N * 4 <= ws << 20 and wide and tile != 1, r
            if word // 100 % 100 == 0:                                  # the policy chose the split itself
                assert K // ksplit >= 512 and cls != PRE_ADD, r
        if cls == ROWSUM:
            assert tile == 4 and ksplit == 1, r
        if cls in (GLU_BWD, ACT_BWD, PAIR2):
            assert tile != 1, r
