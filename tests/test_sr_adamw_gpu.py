"""yat_adamw_sr_step (csrc/optim.hip adamw_sr_kernel) and ``FlatAdamW(stochastic_rounding=True)`` on the GPU.

Bit-exact part: inputs on which every fp32 operation of the step is EXACT, so that neither an fma contraction nor the order of
two roundings can matter, compared as int16 views with the numpy restatement tests/sr_adamw_ref.py.
  case A (parameter path): step 1, betas (0.5, 0.75), eps 0, wd 0, m = v = 0, g any non-zero bf16, p bf16 in [0.5, 2), lr a power
    of two.  m = g / 2 (representable: comes back unchanged), v = g^2 / 4 (16 mantissa bits: the rounding decides), the
    denominator is |g|, the update -+lr (p -+ lr has up to 17 bits: the rounding decides).  A clip coefficient of 0.5 keeps all
    of it exact.  The shadow (decay 0.75) is bf16 in [0.5, 2): s - (s - p_stored) / 4 is a multiple of 2^-10 below 2.
  case B (moment path): lr 0, same betas, p, m, g, s in {k / 256, |k| <= 255} (p, s non-zero), v in {k / 256, 1 <= k <= 255}:
    p comes back bit for bit, m = (m + g) / 2 and v = 3 v / 4 + g^2 / 4 are exact with 9 ... 20 bits.
General inputs are held to a float64 evaluation of the same step: strictly within one bf16 ulp x (1 + 2^-10) -- the result is a
neighbour of the fp32 value, and the fp32 value is within 2^-20 ulp-fractions of the float64 one for these inputs (no clip
coefficient, so g - m is exact and every later rounding is relative to a sum without cancellation)."""
import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_adamw_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF, DEV = torch.bfloat16, "cuda"
BETAS = (0.5, 0.75)
NAMES = ("p", "m", "v", "s")


@pytest.fixture(scope="module")
def ops():
    from yat_amd import ops as o
    o._lib()
    return o


# ------------------------------------------------------------------------------------------------ helpers
def _bits(x):
    """float32 numpy values that are bf16-representable -> bit patterns."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any()
    return (u >> np.uint32(16)).astype(np.uint16)


def _dev(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).to(DEV).view(BF)


def _host(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def _case_a(n, seed, ema):
    rng = np.random.default_rng(seed)
    g = R.rne_bf16(rng.standard_normal(n).astype(np.float32))
    g = np.where((g & 0x7FFF) == 0, np.uint16(0x3F80), g)                      # non-zero
    p = R.rne_bf16(rng.uniform(0.5, 1.99, n).astype(np.float32))
    s = R.rne_bf16(rng.uniform(0.5, 1.99, n).astype(np.float32)) if ema else None
    z = np.zeros(n, dtype=np.uint16)
    return dict(p=p, g=g, m=z, v=z.copy(), s=s)


def _case_b(n, seed, ema):
    rng = np.random.default_rng(seed)
    k = lambda lo, hi: (rng.integers(lo, hi + 1, n) / 256.0).astype(np.float32)
    nz = lambda: k(1, 255) * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n)
    return dict(p=_bits(nz()), g=_bits(k(-255, 255)), m=_bits(k(-255, 255)), v=_bits(k(1, 255)), s=_bits(nz()) if ema else None)


def _launch(ops, st, coef, lr, betas, eps, wd, step, ema_decay, seed, rng_step, elem_offset, lo=0, hi=None, zero_grad=False):
    """One call over [lo, hi) of the device state ``st`` (dict of bf16 tensors, s may be None)."""
    hi = st["p"].numel() if hi is None else hi
    c = None if coef is None else torch.tensor([coef], dtype=torch.float32, device=DEV)
    ops.adamw_sr_step(st["p"][lo:hi], st["g"][lo:hi], st["m"][lo:hi], st["v"][lo:hi], c, lr, betas[0], betas[1], eps, wd, step,
                      zero_grad=zero_grad, ema_shadow=None if st["s"] is None else st["s"][lo:hi], ema_decay=ema_decay, seed=seed,
                      rng_step=rng_step, elem_offset=elem_offset)


def _to_dev(case):
    return {k: (None if b is None else _dev(b)) for k, b in case.items()}


def _ref(case, coef, lr, step, ema_decay, seed, rng_step, elem_offset, betas=BETAS, eps=0.0, wd=0.0, threads=1):
    n = case["p"].size

    def part(lo, hi):
        return R.adamw_sr_ref(case["p"][lo:hi], case["g"][lo:hi], case["m"][lo:hi], case["v"][lo:hi], coef, lr, betas[0], betas[1],
                              eps, wd, step, ema=None if case["s"] is None else case["s"][lo:hi], ema_decay=ema_decay, seed=seed,
                              rng_step=rng_step, elem_offset=elem_offset + lo)
    if threads == 1:
        return part(0, n)
    cuts = list(range(0, n, 1 << 21)) + [n]                    # (the restatement is elementwise in the global index)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda ab: part(*ab), zip(cuts[:-1], cuts[1:])))
    return tuple(None if parts[0][i] is None else np.concatenate([q[i] for q in parts]) for i in range(4))


def _assert_bits(st, want, g_before, what):
    torch.cuda.synchronize()
    for name, w in zip(NAMES, want):
        if w is None:
            assert st[name] is None
            continue
        got = _host(st[name])
        bad = np.flatnonzero(got != w)
        assert bad.size == 0, f"{what}: {name} differs from the restatement at {bad.size} of {w.size} elements, first {bad[:4]}: " \
                              f"{got[bad[:4]]} against {w[bad[:4]]}"
    assert np.array_equal(_host(st["g"]), g_before), f"{what}: the gradients were written"


# ------------------------------------------------------------------------------------------------ exact cases
N_RAGGED = 8 * (256 * 3 + 5)
N_WRAP = (1 << 24) + 2400
BIG_SEED = 0x9E3779B97F4A7C15

# (id, case, n, ema, lr, coef, step, seed, rng_step, elem_offset)
EXACT = [
    ("a_one_vector", "a", 8, True, 2.0 ** -12, None, 1, 0, 1, 0),
    ("a_ragged_lr_2m10", "a", N_RAGGED, False, 2.0 ** -10, None, 1, 1, 1, 0),
    ("a_ragged_lr_2m15_clip_ema", "a", N_RAGGED, True, 2.0 ** -15, 0.5, 1, BIG_SEED, 5, 8 * 1001),
    ("a_pair_high_word", "a", 128, True, 2.0 ** -12, None, 1, 7, 3, (1 << 33) - 64),
    ("b_ragged_ema", "b", N_RAGGED, True, 0.0, None, 2, 3, 9, 0),
    ("b_ragged_clip", "b", N_RAGGED, False, 0.0, 0.5, 1, 3, 9, 64),
    ("b_rng_step_high_word", "b", N_RAGGED, True, 0.0, None, 1, BIG_SEED, (1 << 32) + 3, 0),
    ("b_second_grid_pass", "b", N_WRAP, False, 0.0, None, 1, 11, 2, 0),
    ("a_second_grid_pass_ema", "a", N_WRAP, True, 2.0 ** -12, None, 1, 12, 4, 1 << 20),
]


@pytest.mark.parametrize("case, n, ema, lr, coef, step, seed, rng_step, elem_offset", [e[1:] for e in EXACT], ids=[e[0] for e in EXACT])
def test_exact_inputs_match_the_restatement_bit_for_bit(ops, case, n, ema, lr, coef, step, seed, rng_step, elem_offset):
    data = (_case_a if case == "a" else _case_b)(n, seed=n % 1000 + step, ema=ema)
    st = _to_dev(data)
    _launch(ops, st, coef, lr, BETAS, 0.0, 0.0, step, 0.75, seed, rng_step, elem_offset)
    want = _ref(data, coef, lr, step, 0.75, seed, rng_step, elem_offset, threads=8 if n > (1 << 22) else 1)
    _assert_bits(st, want, data["g"], f"case {case} n={n}")
    got_p, got_m = _host(st["p"]), _host(st["m"])
    if case == "a":
        half_g = R.rne_bf16(R.bf16_to_f32(data["g"]) * np.float32(0.5 if coef is None else 0.25))
        assert np.array_equal(got_m, half_g), "m = g / 2 is representable and must come back unchanged"
        moved = (got_p != data["p"]).mean()
        assert n < 1000 or 0.0 < moved < 1.0, "the rounding of p -+ lr must go both ways"
        print(f"[sr] case a n={n} lr={lr}: {moved:.4f} of the parameters moved")
    else:
        assert np.array_equal(got_p, data["p"]), "lr = 0 must leave the parameters bit for bit"
        assert (got_m != data["m"]).any()


def test_zero_grad_clears_the_gradients_and_nothing_else(ops):
    data = _case_b(N_RAGGED, seed=21, ema=True)
    st = _to_dev(data)
    _launch(ops, st, None, 0.0, BETAS, 0.0, 0.0, 1, 0.75, 4, 6, 0, zero_grad=True)
    want = _ref(data, None, 0.0, 1, 0.75, 4, 6, 0)
    _assert_bits(st, want, np.zeros_like(data["g"]), "zero_grad")


@pytest.mark.parametrize("k", [8, 8 * 257])
def test_slicing_invariance(ops, k):
    """One call over [0, n) = calls over [0, k) and [k, n) with elem_offset = k; elements outside a call's slice keep their bits."""
    n, off = N_RAGGED, 8 * 40
    data = _case_a(n, seed=33, ema=True)
    args = (0.5, 2.0 ** -12, BETAS, 0.0, 0.0, 1, 0.75, 99, 17)
    whole, parts = _to_dev(data), _to_dev(data)
    _launch(ops, whole, *args, off)
    _launch(ops, parts, *args, off + k, lo=k)
    torch.cuda.synchronize()
    for name in NAMES:
        assert np.array_equal(_host(parts[name])[:k], data[name][:k]), f"{name}: a call over [k, n) wrote below k"
    _launch(ops, parts, *args, off, hi=k)
    want = _ref(data, 0.5, 2.0 ** -12, 1, 0.75, 99, 17, off)
    _assert_bits(whole, want, data["g"], "one call")
    _assert_bits(parts, want, data["g"], f"two calls cut at {k}")


def test_same_arguments_same_bits_other_stream_other_bits(ops):
    n = N_RAGGED
    data = _case_a(n, seed=35, ema=True)

    def run(seed, rng_step):
        st = _to_dev(data)
        _launch(ops, st, None, 2.0 ** -12, BETAS, 0.0, 0.0, 1, 0.75, seed, rng_step, 0)
        torch.cuda.synchronize()
        return {k: _host(st[k]) for k in NAMES}
    first, again, other_step, other_seed = run(5, 1), run(5, 1), run(5, 2), run(6, 1)
    for name in NAMES:
        assert np.array_equal(first[name], again[name]), name
        if name == "m":
            continue                                   # m = g / 2 is representable: no draw can change it
        for other in (other_step, other_seed):
            differ = (first[name] != other[name]).mean()
            # two independent draws differ with probability 2 f (1 - f), f the fractional position: p -+ 2^-12 sits at 1 / 16
            # (p below 1) or 1 / 32 of an ulp -> 0.06 ... 0.12; v and s spread over the whole ulp -> about 1 / 3
            assert 0.03 < differ < 0.6, f"{name}: {differ:.3f} of the elements differ under another rng_step / seed"


# ------------------------------------------------------------------------------------------------ general inputs
def _general(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda std: torch.randn(n, generator=gen, device=DEV) * std
    p, g, m = r(0.02).to(BF), r(0.01).to(BF), r(0.01).to(BF)
    v = (r(0.01) ** 2 + 1e-12).to(BF)
    s = (p.float() + r(0.001)).to(BF)
    return dict(p=p, g=g, m=m, v=v, s=s)


def test_general_inputs_stay_within_one_ulp_of_float64(ops):
    n, hyp = 1 << 20, dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, wd=0.01, step=3)
    st = _general(n, 41)
    before = {k: _host(t) for k, t in st.items()}
    assert np.isfinite(R.bf16_to_f32(before["g"])).all() and (R.bf16_to_f32(before["v"]) > 0).all()
    _launch(ops, st, None, hyp["lr"], hyp["betas"], hyp["eps"], hyp["wd"], hyp["step"], 0.999, 77, hyp["step"], 0)
    torch.cuda.synchronize()
    got = {k: _host(st[k]) for k in NAMES}
    truth = R.adamw_sr_ref(before["p"], before["g"], before["m"], before["v"], None, hyp["lr"], *hyp["betas"], hyp["eps"], hyp["wd"],
                           hyp["step"], ema=before["s"], ema_decay=0.999, dtype=np.float64, rounded=False, p_stored=got["p"])
    for name, t in zip(NAMES, truth):
        out = R.bf16_to_f32(got[name]).astype(np.float64)
        assert np.isfinite(out).all() and (t != 0).all(), name
        ulp = np.exp2(np.floor(np.log2(np.abs(t))) - 7)                       # bf16: 8 significant bits
        dist = np.abs(out - t) / ulp
        rne = np.abs(R.bf16_to_f32(R.rne_bf16(t.astype(np.float32))).astype(np.float64) - t) / ulp
        print(f"[sr] general {name}: largest distance to float64 {dist.max():.6f} ulp (round to nearest: {rne.max():.6f}); "
              f"{(dist > 0.5).mean():.4f} of the elements went to the farther neighbour; mean signed error {((out - t) / ulp).mean():+.5f} ulp")
        assert (dist < 1.0 + 2.0 ** -10).all(), f"{name}: {int((dist >= 1.0 + 2.0 ** -10).sum())} elements a whole ulp or more from float64"
        assert abs(((out - t) / ulp).mean()) < 5 * 0.5 / math.sqrt(n) + 1e-4, f"{name}: the rounding is biased"


@pytest.mark.parametrize("bad", ["nan", "+inf", "-inf"])
def test_nonfinite_gradients_follow_the_master_kernel(ops, bad):
    """Non-finite outputs are those of yat_adamw_master_step on the same values, rounded to bf16: same NaN positions, same
    infinities; the finite rest keeps the one-ulp bar of its float32 neighbours."""
    n, hyp = 8 * 773, (1e-5, 0.9, 0.999, 1e-8, 0.01, 3)
    st = _general(n, 43)
    where = torch.tensor([0, 7, 8, 1001, n - 1], device=DEV)
    st["g"][where] = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}[bad]
    w, m32, v32, s32, p16, g16 = st["p"].float(), st["m"].float(), st["v"].float(), st["s"].float(), st["p"].clone(), st["g"].clone()
    ops.adamw_master_step(p16, w, g16, m32, v32, None, *hyp, zero_grad=False, ema_shadow=s32, ema_decay=0.999)
    _launch(ops, st, None, hyp[0], hyp[1:3], hyp[3], hyp[4], hyp[5], 0.999, 1, 3, 0)
    torch.cuda.synchronize()
    for name, ref32 in zip(NAMES, (w, m32, v32, s32)):
        ref, got = ref32.to(BF), st[name]
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{bad} {name}: NaN positions differ from the master kernel's"
        assert torch.equal(torch.isinf(got), torch.isinf(ref)), f"{bad} {name}: infinities differ from the master kernel's"
        nonfinite = ~torch.isfinite(ref)
        assert nonfinite[where].all() and int(nonfinite.sum()) == where.numel(), f"{bad} {name}"
        inf = torch.isinf(ref)
        assert torch.equal(got[inf].view(torch.int16), ref[inf].view(torch.int16))
        fin = ~nonfinite
        assert ((got[fin].float() - ref32[fin]).abs() <= ref32[fin].abs() * 2.0 ** -7).all(), f"{bad} {name}: a finite element moved"


# ------------------------------------------------------------------------------------------------ FlatAdamW on the device
def _up(x, a):
    return -(-x // a) * a


def _flat_stand_in(seed, **extra):
    """The five-tensor, two-bucket flat layout of tests/test_master_adamw_gpu.py (bucket lengths are multiples of 64)."""
    numel, buckets = [96 * 40, 40, 3 * 3 * 16, 2000, 8], [[0, 1], [2, 3, 4]]
    starts, lows, off = [], [], 0
    for b in buckets:
        off = _up(off, 64)
        lows.append(off)
        for t in b:
            starts.append(off)
            off += _up(numel[t], 8)
    off = _up(off, 64)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    flat = (torch.randn(off, generator=gen, device=DEV) * 0.02).to(BF)
    return SimpleNamespace(flat_param=flat, flat_grad=torch.zeros(off, dtype=BF, device=DEV),
                           seg_start=torch.tensor(starts + [off], dtype=torch.int64), numel_flat=off,
                           bucket_bounds=list(zip(lows, lows[1:] + [off])), param_events=None,
                           join_pending_update=torch.cuda.synchronize, **extra)


class _FakeDDP:
    """One rank of a data-parallel job emulated in one process: collectives are stitched by hand from the other ranks' tensors."""

    def __init__(self, ops, rank, world_state):
        self.ops, self.rank, self.ws = ops, rank, world_state

    def allreduce_bulk(self, partial, mean=False):
        assert not mean
        for q, (model, opt) in enumerate(self.ws):
            if q == self.rank:
                continue                                           # add what rank q holds: the sums of the pieces it owns
            theirs = torch.zeros_like(partial)
            self.ops.gradnorm_pieces_partial(model.flat_grad, opt._piece_start, opt._chunk_base, opt._max_chunks,
                                             opt._owned_mask(model.shard), theirs)
            partial.add_(theirs)

    def allgather_bulk(self, t):
        model, opt = self.ws[self.rank]
        for name, base in (("flat_param", model.flat_param), ("ema_shadow", opt.ema_shadow)):
            if base is not None and base.data_ptr() <= t.data_ptr() < base.data_ptr() + base.numel() * 2:
                lo = (t.data_ptr() - base.data_ptr()) // 2
                self.pending.append((name, lo, lo + t.numel()))
                return
        raise AssertionError("all-gather of an unknown buffer")


def _flush_gathers(ws):
    """Deliver the recorded all-gathers: slice q of every gathered range comes from rank q."""
    world = len(ws)
    todo = [set(m.shard.ddp.pending) for m, _ in ws]
    assert all(t == todo[0] for t in todo), "the ranks gathered different ranges"
    torch.cuda.synchronize()
    for name, lo, hi in sorted(todo[0]):
        s_ = (hi - lo) // world
        for q in range(world):
            src = getattr(ws[q][0] if name == "flat_param" else ws[q][1], name)[lo + q * s_:lo + (q + 1) * s_]
            for r in range(world):
                if r != q:
                    getattr(ws[r][0] if name == "flat_param" else ws[r][1], name)[lo + q * s_:lo + (q + 1) * s_].copy_(src)
    for m, _ in ws:
        m.shard.ddp.pending = []


@pytest.mark.parametrize("sharded_overlap", [False, True], ids=["sharded_serial", "sharded_overlap"])
def test_flat_adamw_paths_give_identical_bits(ops, sharded_overlap, monkeypatch):
    """The overlapped per-bucket update, the single call and a two-rank sharded step: same parameters, moments and shadow, and
    the single call is the direct kernel call at (sr_seed, the optimizer's step count, offset 0) with the optimizer's clip."""
    from yat_amd.optim import FlatAdamW
    monkeypatch.delenv("YAT_MASTER_WEIGHTS", raising=False)
    monkeypatch.delenv("YAT_STOCHASTIC_ROUNDING", raising=False)
    kw = dict(lr=1e-4, weight_decay=0.01, max_grad_norm=1.0, use_ema=True, ema_decay=0.999, stochastic_rounding=True, sr_seed=1234)
    single_m, overlap_m = _flat_stand_in(51), _flat_stand_in(51)
    single, overlap = FlatAdamW(single_m, overlap_update=False, **kw), FlatAdamW(overlap_m, overlap_update=True, **kw)
    assert overlap.overlap_update and not single.overlap_update and single.exp_avg.dtype == BF and single.master is None
    ws = []
    for r in range(2):
        model = _flat_stand_in(51)
        ws.append((model, None))
        model.shard = SimpleNamespace(ddp=_FakeDDP(ops, r, ws), rank=r, world=2)
        model.shard.ddp.pending = []
        ws[r] = (model, FlatAdamW(model, overlap_update=sharded_overlap, **kw))
    n = single_m.numel_flat
    gen = torch.Generator(device=DEV).manual_seed(52)
    for step in range(1, 4):
        grad = (torch.randn(n, generator=gen, device=DEV) * (1.0 if step != 2 else 1e-3)).to(BF)      # clipped, not clipped, clipped
        for model in (single_m, overlap_m, ws[0][0], ws[1][0]):
            model.flat_grad.copy_(grad)
        twin = dict(p=single_m.flat_param.clone(), g=grad.clone(), m=single.exp_avg.clone(), v=single.exp_avg_sq.clone(),
                    s=single.ema_shadow.clone())
        single.step()
        overlap.step()
        for _, opt in ws:
            opt.step()
        _flush_gathers(ws)
        for _, opt in ws:
            assert opt.gather_ema()
        _flush_gathers(ws)
        torch.cuda.synchronize()
        assert (single.clip_coef.item() < 1.0) == (step != 2)
        ops.adamw_sr_step(twin["p"], twin["g"], twin["m"], twin["v"], single.clip_coef, 1e-4, 0.9, 0.999, 1e-8, 0.01, step,
                          zero_grad=False, ema_shadow=twin["s"], ema_decay=single._ema_decay_now(), seed=1234, rng_step=step,
                          elem_offset=0)
        torch.cuda.synchronize()
        want = dict(flat_param=twin["p"], exp_avg=twin["m"], exp_avg_sq=twin["v"], ema_shadow=twin["s"])
        runs = [("single call", single_m, single), ("overlapped buckets", overlap_m, overlap), ("rank 0", *ws[0]), ("rank 1", *ws[1])]
        for what, model, opt in runs:
            assert opt.step_count == step
            assert torch.equal(opt.clip_coef, single.clip_coef), f"step {step} {what}: clip coefficient"
            for name, w in want.items():
                got = getattr(model if name == "flat_param" else opt, name)
                if what.startswith("rank") and name.startswith("exp_avg"):
                    r = opt.model.shard.rank                      # a rank's moments are current on its own slices only
                    for lo, hi in model.bucket_bounds:
                        s_ = (hi - lo) // 2
                        sl = slice(lo + r * s_, lo + (r + 1) * s_)
                        assert torch.equal(got[sl].view(torch.int16), w[sl].view(torch.int16)), f"step {step} {what}: {name}"
                    continue
                assert torch.equal(got.view(torch.int16), w.view(torch.int16)), f"step {step} {what}: {name} differs from the direct call"
    assert (overlap_m.param_events is not None) and single_m.param_events is None
    assert not torch.equal(single_m.flat_param, _flat_stand_in(51).flat_param)


def test_flat_adamw_range_update_uses_the_optimizers_own_step_for_the_bits(ops, monkeypatch):
    """``update_ranges`` hands each range its own bias-correction step; the random stream still follows ``step_count``, and the
    elements outside the range keep their bits."""
    from yat_amd.optim import FlatAdamW
    monkeypatch.delenv("YAT_MASTER_WEIGHTS", raising=False)
    model = _flat_stand_in(61)
    n = model.numel_flat
    opt = FlatAdamW(model, lr=1e-4, weight_decay=0.0, max_grad_norm=None, use_ema=True, stochastic_rounding=True, sr_seed=9)
    model.update_ranges = lambda: [(8, n - 8, 1)]                  # a range that is always at its first step
    gen = torch.Generator(device=DEV).manual_seed(62)
    for step in (1, 2):
        grad = (torch.randn(n, generator=gen, device=DEV) * 0.01).to(BF) if step == 1 else model.flat_grad.clone()
        model.flat_grad.copy_(grad)
        twin = dict(p=model.flat_param.clone(), g=grad.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(), s=opt.ema_shadow.clone())
        opt.step()
        _launch(ops, twin, None, 1e-4, (0.9, 0.999), 1e-8, 0.0, 1, opt._ema_decay_now(), 9, step, 8, lo=8, hi=n - 8)
        torch.cuda.synchronize()
        for name, got in (("p", model.flat_param), ("m", opt.exp_avg), ("v", opt.exp_avg_sq), ("s", opt.ema_shadow)):
            assert torch.equal(got.view(torch.int16), twin[name].view(torch.int16)), f"step {step}: {name}"
    assert opt.step_count == 2
