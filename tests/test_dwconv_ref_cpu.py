"""The case table of test_dwconv_gpu.py reaches every walk, band and edge it is meant to, its inputs keep every sum exact, and
its checker bites -- CPU.

tests/dwconv_ref.py holds the table, plan() (the launchers' arithmetic), the input builder, the fp64 model and check().  Here:
coverage  plan() classifies every case as the table says, and over the table every class is reached: the streaming forward at
          R = 2, 3, 4, 5, 8 with at least three steps, with several groups per image and with one, a ragged last step, a last
          group shorter than the others, idle run slots, a channel tail; each of the five band kernels with bpb >= 2, at least
          two groups and a ragged last band; the three direct kernels.  The finding behind the table is asserted as well: every
          shape of test_dwconv_glu_fwd_bwd that takes the streaming forward walks its ring one step.
validity  for every case the largest sum of |terms| of every output is below 2^24, and every stored value is an integer of
          magnitude <= 256 or one rounding of an exact integer.  Large cases run at reduced_channels(Hc) <= 128 channels with the
          same Hc % 64 and the geometry plan() gives for the full shape: the sums run over B h w, not over Hc.
bite      a plain-torch executor that computes band by band and step by step, as the kernels address memory, passes every
          case; with each planted error of dwconv_ref.FAULTS at least one case fails torch.equal or the guard check.
Nothing here touches yat_amd.
"""
import pytest
import torch

from tests import dwconv_ref as R


def _small(case):
    return (case.B, case.h, case.w, R.reduced_channels(case.Hc))


@pytest.fixture(scope="module")
def built():
    out = {}
    for c in R.TABLE:
        dims = _small(c)
        inp = R.build(dims, seed=1)
        out[c.name] = (R.plan(*c.dims), dims, inp, R.model(dims, inp))
    return out


def _run(case, built, fault=None, calls="f12a"):
    """-> failures of check() for the CPU executor on one case, over the calls the GPU file makes"""
    geo, dims, inp, m = built[case.name]
    M, C2 = dims[0] * dims[1] * dims[2], 2 * dims[3]
    fails = []

    def chk(name, got, want):
        fails.extend(R.check(dims, f"{case.name} {name}", got, want))

    if "f" in calls:
        W = R.windows(dims, "cpu")
        R.cpu_fwd(geo, dims, inp, W["y"], W["u"], fault)
        chk("y", W["y"], m.y)
        chk("u", W["u"], m.u)
        if fault is None:
            W2 = R.windows(dims, "cpu")
            R.cpu_fwd(geo, dims, inp, W2["y"])
            assert torch.equal(W2["y"].buf.view(torch.int16), W["y"].buf.view(torch.int16))
            assert W2["u"].guards_intact() and (W2["u"].view.view(torch.int16) == R.GUARD_BITS).all()
    if "1" in calls:
        W = R.windows(dims, "cpu")
        du_ws = torch.full((M, C2), R.GUARD_BITS, dtype=torch.int16).view(R.BF)
        R.cpu_bwd(geo, dims, inp, W["dz"], W["dw"], W["db"], du_ws, fault=fault)
        chk("du(dy)", du_ws, m.du1)
        chk("dz(dy)", W["dz"], m.dz1)
        chk("dw(dy)", W["dw"], m.dw1)
        chk("db(dy)", W["db"], m.db1)
    for key, acc in (("2", False), ("a", True)):
        if key not in calls:
            continue
        prev = dict(dw=inp.prev_dw, db=inp.prev_db, dzs=inp.prev_dzs) if acc else None
        want = m.accum if acc else m.plain
        W = R.windows(dims, "cpu", prev=prev)
        R.cpu_bwd(geo, dims, inp, W["dz"], W["dw"], W["db"], None, accumulate=acc, dzs=W["dzs"], du=inp.du, fault=fault)
        tag = "du=,acc" if acc else "du="
        chk(f"dz({tag})", W["dz"], m.dz2)
        for k in ("dw", "db", "dzs"):
            chk(f"{k}({tag})", W[k], want[k])
    return fails


# ------------------------------------------------------------------------------------------------ coverage
@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_plan_classifies_the_case(case):
    p = R.plan(*case.dims)
    for entry, want in case.want.items():
        got = {k: p[entry].get(k) for k in want}
        assert got == want, (case.name, entry, p[entry])
    if case.group == "stream3":                               # groups start mid-image; the last is shorter and ends ragged
        f = p["fwd"]
        assert f["nchunk"] * case.B == 200 and f["ragged"] == (False, False, True) and f["rpg"] == 3 * f["R"]
    if case.group == "stream1":
        f = p["fwd"]
        assert f["nchunk"] * case.B == 600 and f["ragged"] == (True,) and f["rpg"] >= case.h
    if case.group == "band":
        for entry in case.want:
            e = p[entry]
            assert e["bpb"] >= 2 and e["ngrp"] >= 2 and e["last_band_rows"] == 1 and e["nbands"] % e["bpb"], (case.name, entry)
    # one [M, 2Hc] array stays below 50 MB, and every dynamic-LDS request inside its kernel's budget
    assert case.B * case.h * case.w * 2 * case.Hc * 2 < 50e6
    assert all(e.get("lds", 0) <= R.lds_budget(2) for e in p.values())


def test_table_reaches_every_class(capsys):
    plans = [(c, R.plan(*c.dims)) for c in R.TABLE]
    stream = [(c, p["fwd"]) for c, p in plans if p["fwd"]["kernel"] == "stream"]
    multi = [f for _, f in stream if min(f["steps"]) >= 2 and max(f["steps"]) >= 3]
    with capsys.disabled():
        print(f"\n[dwconv exact] {len(R.TABLE)} cases")
        for c, p in plans:
            print(f"[dwconv exact] {c.name}: " + "; ".join(
                f"{k} {e['kernel']}" + "".join(f" {n}={e[n]}" for n in ("R", "rpg", "steps", "idle", "nbands", "bpb", "ngrp",
                                                                         "nrg", "nsb", "nx", "tail") if e.get(n) is not None)
                for k, e in p.items()))
    assert {f["R"] for f in multi if max(f["steps"]) >= 3} == {2, 3, 4, 5, 8}
    assert {f["R"] for f in multi if f["ngrp"] >= 2} == {2, 3, 4, 5, 8}
    assert {f["R"] for f in multi if f["ngrp"] == 1} >= {2, 3, 5}
    assert any(max(f["steps"]) >= 4 for f in multi)                                 # the ring index wraps twice
    assert all(any(f["ragged"]) for f in multi)                                      # a ragged last step
    assert any(f["steps"][-1] < f["steps"][0] for f in multi)                       # a last group shorter than the others
    assert {f["idle"] for f in multi} >= {0, 1, 2}
    assert any(f["tail"] for f in multi) and any(not f["tail"] for f in multi)
    for entry, kernels in (("fwd", ("tile64x3", "tile64x2")), ("pass1", ("tile32x3",)), ("pass2", ("bwd2_gz64", "bwd2_lds32"))):
        for k in kernels:
            hard = [c.name for c, p in plans if p[entry]["kernel"] == k and p[entry]["bpb"] >= 2 and p[entry]["ngrp"] >= 2
                    and p[entry]["last_band_rows"] < p[entry]["R"]]
            assert hard, (entry, k)
            assert any(p[entry]["kernel"] == k and p[entry]["bpb"] == 1 for c, p in plans), (entry, k)   # and the plain walk
    for entry in ("fwd", "pass1", "pass2"):
        assert any(p[entry]["kernel"] == "direct" for _, p in plans), entry
    d = next(p for c, p in plans if c.group == "direct")
    assert d["fwd"]["nx"] == 2 and d["pass2"]["last_group_rows"] == 2 and 70 % (4 * R.SEG) != 0
    # single-step streams stay in the table too (the old small shapes)
    assert any(f["steps"] == (1,) for _, f in stream)


def test_old_table_walks_the_ring_one_step_only():
    """the finding: no shape of test_kernels_gpu.py::test_dwconv_glu_fwd_bwd takes the streaming forward past its first step"""
    took_stream = []
    for dims in R.OLD_SMALL + R.OLD_LARGE:
        f = R.plan(*dims)["fwd"]
        if f["kernel"] == "stream":
            took_stream.append(dims[1:3])
            assert set(f["steps"]) == {1} and f["rpg"] == f["R"], dims
    assert sorted(took_stream) == sorted([(5, 9), (32, 32), (7, 20), (9, 16), (10, 8), (31, 30)])
    # and what the comment above that test says of its last two shapes
    a, b = (R.plan(*d) for d in R.OLD_LARGE)
    assert (a["fwd"]["kernel"], a["fwd"]["bpb"], a["pass1"]["bpb"], a["pass2"]["kernel"], a["pass2"]["bpb"]) == \
        ("tile64x3", 2, 3, "bwd2_gz64", 3)
    assert (b["fwd"]["kernel"], b["fwd"]["bpb"], b["pass2"]["kernel"], b["pass2"]["bpb"]) == ("tile64x2", 2, "bwd2_lds32", 3)
    # where pass 1 or pass 2 walks several bands there, one group has the whole image: no workgroup starts mid-image
    assert all(p[e]["ngrp"] == 1 for p in (a, b) for e in ("pass1", "pass2") if p[e]["bpb"] > 1)
    assert a["pass1"]["bpb"] > 1 and a["pass2"]["bpb"] > 1 and b["pass2"]["bpb"] > 1


def test_reduced_channels_keep_the_tail():
    for c in R.TABLE:
        r = R.reduced_channels(c.Hc)
        assert r <= 128 and (r == c.Hc or r > 64) and r % 64 == c.Hc % 64, c.name


# ------------------------------------------------------------------------------------------------ validity
def _is_int(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_every_sum_is_exact(case, built):
    _, dims, inp, m = built[case.name]
    # whatever is drawn, a new case stays below 47 * 146 per pixel term at any channel count: 960 pixels at the most
    assert case.group == "old" or 47 * 146 * case.B * case.h * case.w < 6.6e6
    for name, bound in m.bounds.items():
        assert bound < R.EXACT_LIMIT, (case.name, name, bound)
    # stored as they are: integers of at most 8 significant bits
    for name, t in (("u", m.u), ("du", m.du1)):
        assert _is_int(t) and t.abs().max() <= 256, (case.name, name)
    # stored after one rounding of an exact integer
    for name, exact, stored in (("y", m.y_exact, m.y), ("dz(dy)", m.dz1_exact, m.dz1), ("dz(du=)", m.dz2_exact, m.dz2)):
        assert _is_int(exact) and exact.abs().max() < R.EXACT_LIMIT and torch.equal(R.rb(exact), stored), (case.name, name)
    for sums in (m.sums1, m.sums2):
        for name, t in sums.items():
            assert _is_int(t) and t.abs().max() < R.EXACT_LIMIT, (case.name, name)
    for t in (inp.prev_dw, inp.prev_db, inp.prev_dzs, inp.s, inp.z, inp.wdw, inp.bdw, inp.dy, inp.du):
        assert _is_int(t.double()) and t.double().abs().max() <= 256
    # the inputs are what the docstring of dwconv_ref says: nine distinct taps, live and dead values of both kinds present
    assert (inp.wdw.double().sort(1).values == torch.tensor([-4., -3, -2, -1, 1, 2, 3, 4, 5]).double()).all()
    g = inp.bdw.double()[dims[3]:]
    assert set(g.tolist()) == {float(R.G_LIVE), float(R.G_DEAD)}
    z = inp.z.double()
    live = (z >= R.Z_LIVE[0]) & (z <= R.Z_LIVE[1])
    dead = (z >= R.Z_DEAD[0]) & (z <= R.Z_DEAD[1])
    assert (live | dead).all() and live.any() and dead.any()
    ug = m.u[:, dims[3]:]
    assert (((ug >= 46) & (ug <= 146)) | ((ug >= -230) & (ug <= -130))).all()
    # something to see: the outputs are not mostly zero
    for t in (m.y, m.dz1, m.dz2, m.dw1, m.plain["dw"], m.plain["dzs"]):
        assert (t != 0).double().mean() > 0.1


def test_window_guards():
    W = R.Win((3, 5), 7, "cpu")
    assert W.off == 128 and W.buf.numel() == 271 and W.guards_intact()
    assert (W.view.view(torch.int16) == R.GUARD_BITS).all() and torch.isfinite(W.buf.float()).all()
    W.view.fill_(1.0)
    assert W.guards_intact()
    W.buf[W.off + W.n] = 1.0
    assert not W.guards_intact()
    W = R.Win((4,), 1, "cpu")
    W.buf[W.off - 1] = 0.0
    assert not W.guards_intact()
    assert R.check((1, 1, 1, 2), "x", torch.tensor([-0.0, 1.0]), torch.tensor([0.0, 1.0])) == []
    assert R.check((1, 1, 1, 2), "x", torch.tensor([0.0, 1.0]), torch.tensor([0.0, 1.0078125]))


# ------------------------------------------------------------------------------------------------ the checker bites
def test_correct_executor_passes_every_case(built):
    bad = {c.name: f for c in R.TABLE if (f := _run(c, built))}
    assert not bad, bad


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_error_is_caught(fault, built):
    caught = []
    for c in R.TABLE:
        fails = _run(c, built, fault, R.FAULT_CALLS[fault])
        if fails:
            caught.append((c.name, fails[0]))
            break                                             # one would do; the table is not walked to its end for a count
    print(f"[dwconv exact] {fault}: {caught}")
    assert caught, fault


@pytest.mark.parametrize("case", [c for c in R.TABLE if c.group == "band"], ids=lambda c: c.name)
def test_band_cases_report_their_own_kernel(case, built):
    """the multi-band cases see a zeroed bottom halo in the output of each band kernel they are in the table for, and the
    weight gradient that misses the one-row last band although dz is whole"""
    halo = _run(case, built, "halo_bottom_zero", "f12")
    for entry, output in (("fwd", " y:"), ("pass1", " du(dy):"), ("pass2", " dw(du=):")):
        if entry in case.want:
            assert any(output in f for f in halo), (case.name, entry, halo)
    if "pass2" in case.want:
        last = _run(case, built, "dw_miss_last_band", "2")
        assert any(" dw(du=):" in f for f in last) and not any(" dz(du=):" in f for f in last), (case.name, last)
