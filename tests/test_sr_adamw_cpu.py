"""Stochastic-rounding optimizer mode, the parts that need no GPU: Philox4x32 known answers, the properties of the rounding rule
on the numpy restatement (tests/sr_adamw_ref.py), that sub-ulp sums accumulate, the C entry point's argument checks,
``FlatAdamW``'s state and switches on CPU tensors, and the ``stochastic_rounding`` config key."""
import glob
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_adamw_ref as R  # noqa: E402

from yat_amd import lib as ylib  # noqa: E402
from yat_amd.common.training_parameters_reader import TrainingParameters  # noqa: E402

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ------------------------------------------------------------------------------------------------ Philox known answers
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "5f6fb709 0d893f64 4f121f81 4f730a48"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd", "5207ddc2 45165e59 4d8ee751 8c52f662"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1",
        "4dfccaba 190a87f0 c47362ba b6b5242a")]


@pytest.mark.parametrize("counter, key, want10, want7", KAT)
def test_philox_known_answers(counter, key, want10, want7):
    for rounds, want in ((10, want10), (7, want7)):
        got = " ".join(f"{int(w):08x}" for w in R.philox4x32(counter, key, rounds))
        assert got == want, (rounds, got)


def test_round_count_agrees_with_the_kernel_source():
    import re
    src = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "yat_amd", "csrc", "optim.hip")).read()
    assert int(re.search(r"constexpr int SR_PHILOX_ROUNDS = (\d+);", src).group(1)) == R.PHILOX_ROUNDS
    assert R.PHILOX_ROUNDS in (7, 10)


def test_bit_fields_of_one_call_serve_two_parameters():
    """Pair j = idx >> 1; even parameter (w0, w1), odd (w2, w3); p / exp_avg from the first word, exp_avg_sq / shadow from the second."""
    seed, step, idx = 0x1122334455667788, (1 << 32) + 3, np.array([(1 << 33) + 10, (1 << 33) + 11], dtype=np.uint64)
    j = int(idx[0]) >> 1
    w = [int(x) for x in R.philox4x32((j & 0xFFFFFFFF, j >> 32, 3, 1), (0x55667788, 0x11223344))]
    want = {R.FIELD_P: (w[0] & 0xFFFF, w[2] & 0xFFFF), R.FIELD_EXP_AVG: (w[0] >> 16, w[2] >> 16),
            R.FIELD_EXP_AVG_SQ: (w[1] & 0xFFFF, w[3] & 0xFFFF), R.FIELD_EMA: (w[1] >> 16, w[3] >> 16)}
    for field, pair in want.items():
        assert tuple(int(x) for x in R.sr_bits(seed, step, idx, field)) == pair, field


# ------------------------------------------------------------------------------------------------ rounding properties
N = 65536
IDX = np.uint64(2 ** 32 - 100) + np.arange(N, dtype=np.uint64)         # the pair index's high word changes inside the range
STREAMS = [(0, 1), (1234567890123, 7), (0, 2)]
FRACTIONS = [1 / 256, 1 / 4, 1 / 2, 3 / 4, 255 / 256]


def _neighbours(x):
    """The bf16 neighbours of finite float32 ``x`` as bit patterns: truncation (towards zero) and one step away from zero."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    lo = (u >> np.uint32(16)).astype(np.uint16)
    return lo, np.where((u & np.uint32(0xFFFF)) != 0, lo + np.uint16(1), lo)


@pytest.mark.parametrize("seed, rng_step", STREAMS)
def test_representable_values_are_returned_unchanged(seed, rng_step):
    bits = (np.arange(N, dtype=np.uint32) * np.uint32(40503) >> np.uint32(3)).astype(np.uint16)      # all sorts of bf16 patterns
    bits = np.where((bits & 0x7F80) == 0x7F80, bits & np.uint16(0x807F), bits)                       # finite ones (0, subnormals kept)
    bits[:4] = (0x0000, 0x8000, 0x7F7F, 0xFF7F)                                                      # +-0 stay +-0, +-max stay
    x = R.bf16_to_f32(bits)
    for field in range(4):
        assert np.array_equal(R.sr_bf16(x, seed, rng_step, IDX, field), bits), field
    assert np.array_equal(R.sr_bf16_r(x, np.full(N, 0xFFFF)), bits)


@pytest.mark.parametrize("seed, rng_step", STREAMS)
def test_result_is_always_a_neighbour_and_negatives_mirror(seed, rng_step):
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(N) * np.exp(rng.uniform(-20, 20, N))).astype(np.float32)
    for field in range(4):
        out = R.sr_bf16(x, seed, rng_step, IDX, field)
        lo, hi = _neighbours(x)
        assert np.all((out == lo) | (out == hi)), field
        assert np.any(out != lo) and np.any(out != hi)
        mirrored = R.sr_bf16(-x, seed, rng_step, IDX, field)
        assert np.array_equal(mirrored, out ^ np.uint16(0x8000)), field


@pytest.mark.parametrize("f", FRACTIONS)
@pytest.mark.parametrize("seed, rng_step", STREAMS)
def test_probability_of_rounding_up_is_the_fraction(seed, rng_step, f):
    """x = 1 + f ulp: the count rounded up is within 5 sigma of N f (round to nearest gives 0 or N)."""
    x = np.full(N, 1.0 + f * 2.0 ** -7, dtype=np.float32)
    assert float(x[0]) == 1.0 + f * 2.0 ** -7
    up = int((R.bf16_to_f32(R.sr_bf16(x, seed, rng_step, IDX, R.FIELD_P)) > 1.0).sum())
    sigma = math.sqrt(N * f * (1 - f))
    print(f"[sr] seed {seed} rng_step {rng_step} f {f}: {up} of {N} rounded up, {(up - N * f) / sigma:+.2f} sigma")
    assert abs(up - N * f) <= 5 * sigma
    assert int((R.bf16_to_f32(R.rne_bf16(x)) > 1.0).sum()) in (0, N)
    down = int((R.bf16_to_f32(R.sr_bf16(-x, seed, rng_step, IDX, R.FIELD_P)) < -1.0).sum())
    assert down == up


@pytest.mark.parametrize("seed, rng_step", STREAMS)
def test_non_finite_values_take_the_round_to_nearest_conversion(seed, rng_step):
    pats = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F80FFFF, 0xFF80FFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001],
                    dtype=np.uint32)
    x = np.tile(pats, N // len(pats) + 1)[:N].view(np.float32)
    for field in range(4):
        out = R.sr_bf16(x, seed, rng_step, IDX, field)
        assert np.array_equal(out, R.rne_bf16(x))
        o = R.bf16_to_f32(out)
        assert np.array_equal(np.isnan(o), np.isnan(x)) and np.array_equal(np.signbit(o), np.signbit(x))
        assert np.array_equal(o[np.isinf(x)], x[np.isinf(x)])
    # what round to nearest gives: torch's conversion agrees on +-Inf bit for bit and keeps every NaN a NaN
    t = torch.from_numpy(x.copy()).to(BF).view(torch.int16).numpy().view(np.uint16)
    inf = np.isinf(x)
    assert np.array_equal(t[inf], R.rne_bf16(x)[inf]) and np.isnan(R.bf16_to_f32(t[~inf])).all()


def test_round_to_nearest_restatement_is_torchs_on_finite_values():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(N) * np.exp(rng.uniform(-30, 30, N))).astype(np.float32)
    x[:3] = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.4e38)                   # ties to even, and the overflow to Inf
    t = torch.from_numpy(x).to(BF).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.rne_bf16(x), t)


# ------------------------------------------------------------------------------------------------ accumulation
def test_sub_ulp_sums_accumulate_where_round_to_nearest_stalls():
    """4096 elements at 1.0 take + 2^-12 (1/32 of a bf16 ulp) 1024 times: the mean ends at 1.25 within 0.005 (restatement:
    1.25075; predicted standard deviation of the mean 6.8e-4); round to nearest never leaves 1.0."""
    n, inc = 4096, np.float32(2.0 ** -12)
    idx = np.arange(n, dtype=np.uint64)
    sr = np.full(n, 0x3F80, dtype=np.uint16)
    rn = sr.copy()
    for step in range(1, 1025):
        sr = R.sr_bf16(R.bf16_to_f32(sr) + inc, 5, step, idx, R.FIELD_P)
        rn = R.rne_bf16(R.bf16_to_f32(rn) + inc)
    mean = float(R.bf16_to_f32(sr).astype(np.float64).mean())
    print(f"[sr] mean after 1024 additions of 2^-12: {mean:.5f}")
    assert abs(mean - 1.25) <= 0.005
    assert np.all(rn == 0x3F80)


# ------------------------------------------------------------------------------------------------ C entry point
def test_sr_step_bad_arguments_are_rejected_without_a_gpu(built_lib):
    """yat_adamw_sr_step validates before any launch, so fake non-null pointers are never dereferenced."""
    lib = ylib.load()
    P, EINVAL = 0x7f0000001000, -1
    good = dict(n=64, param=P, grad=P, exp_avg=P, exp_avg_sq=P, step=1, rng_step=1, elem_offset=0)

    def call(**kw):
        a = {**good, **kw}
        return lib.yat_adamw_sr_step(a["n"], a["param"], a["grad"], a["exp_avg"], a["exp_avg_sq"], None, 1e-4, 0.9, 0.999, 1e-8, 0.0,
                                     a["step"], 1, None, 0.0, 0, a["rng_step"], a["elem_offset"], None)

    assert call(n=7) == EINVAL
    assert call(n=0) == EINVAL
    assert call(n=-8) == EINVAL
    assert call(n=(1 << 33) + 4) == EINVAL            # n % 8 is checked on all 64 bits
    assert call(elem_offset=-8) == EINVAL
    assert call(elem_offset=4) == EINVAL
    assert call(elem_offset=(1 << 33) + 4) == EINVAL
    assert call(rng_step=-1) == EINVAL
    assert call(step=0) == EINVAL
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert call(**{name: None}) == EINVAL, name


# ------------------------------------------------------------------------------------------------ FlatAdamW
def _stand_in(**extra):
    """The five-tensor, two-bucket flat layout of tests/test_master_adamw_cpu.py, on the CPU."""
    numel = [96 * 40, 40, 3 * 3 * 16, 2000, 8]
    buckets = [[0, 1], [2, 3, 4]]
    up = lambda x, a: -(-x // a) * a
    starts, lows, off = [], [], 0
    for b in buckets:
        off = up(off, 64)
        lows.append(off)
        for t in b:
            starts.append(off)
            off += up(numel[t], 8)
    off = up(off, 64)
    g = torch.Generator().manual_seed(7)
    return SimpleNamespace(flat_param=(torch.randn(off, generator=g) * 0.5).to(BF), flat_grad=torch.zeros(off, dtype=BF),
                           seg_start=torch.tensor(starts + [off], dtype=torch.int64), numel_flat=off,
                           bucket_bounds=list(zip(lows, lows[1:] + [off])), param_events=None,
                           join_pending_update=lambda: None, **extra)


@pytest.fixture
def clean_env(monkeypatch):
    monkeypatch.delenv("YAT_MASTER_WEIGHTS", raising=False)
    monkeypatch.delenv("YAT_STOCHASTIC_ROUNDING", raising=False)
    return monkeypatch


def test_flat_adamw_sr_state_is_bf16_without_a_master(clean_env):
    from yat_amd.optim import FlatAdamW
    model = _stand_in()
    opt = FlatAdamW(model, lr=1e-5, stochastic_rounding=True, sr_seed=11, use_ema=True)
    assert opt.stochastic_rounding is True and opt.master_weights is False and opt.master is None and opt.sr_seed == 11
    for name in ("exp_avg", "exp_avg_sq", "ema_shadow"):
        assert getattr(opt, name).dtype == BF and getattr(opt, name).shape == (model.numel_flat,), name
    assert torch.equal(opt.ema_shadow, model.flat_param) and opt.ema_shadow.data_ptr() != model.flat_param.data_ptr()
    opt.resync_master()                                       # nothing to do, and no error
    assert FlatAdamW(model, lr=1e-5).stochastic_rounding is False
    assert FlatAdamW(model, lr=1e-5, stochastic_rounding=True).sr_seed == 0


@pytest.mark.parametrize("value, want", [(None, False), ("", False), ("0", False), ("false", False), ("No", False), ("off", False),
                                         ("1", True), ("true", True)])
def test_environment_default(clean_env, value, want):
    from yat_amd.optim import FlatAdamW, stochastic_rounding_default
    if value is not None:
        clean_env.setenv("YAT_STOCHASTIC_ROUNDING", value)
    assert stochastic_rounding_default() is want
    assert FlatAdamW(_stand_in(), lr=1e-5).stochastic_rounding is want
    assert FlatAdamW(_stand_in(), lr=1e-5, stochastic_rounding=None).stochastic_rounding is want
    assert FlatAdamW(_stand_in(), lr=1e-5, stochastic_rounding=not want).stochastic_rounding is (not want)     # an argument wins


@pytest.mark.parametrize("how", ["arguments", "environment", "argument_and_environment", "environment_and_argument"])
def test_master_weights_with_stochastic_rounding_is_refused(clean_env, how):
    from yat_amd.optim import FlatAdamW
    kw = {}
    if how in ("arguments", "argument_and_environment"):
        kw["master_weights"] = True
    else:
        clean_env.setenv("YAT_MASTER_WEIGHTS", "1")
    if how in ("arguments", "environment_and_argument"):
        kw["stochastic_rounding"] = True
    else:
        clean_env.setenv("YAT_STOCHASTIC_ROUNDING", "1")
    with pytest.raises(ValueError, match="stochastic_rounding"):
        FlatAdamW(_stand_in(), lr=1e-5, **kw)
    # an explicit False on either side lifts the conflict
    assert FlatAdamW(_stand_in(), lr=1e-5, **{**kw, "master_weights": False}).stochastic_rounding is True
    assert FlatAdamW(_stand_in(), lr=1e-5, **{**kw, "stochastic_rounding": False}).master_weights is True


def test_sharded_step_is_not_refused(clean_env, built_lib):
    """Unlike master weights the mode has a sharded step: with CPU tensors it gets as far as the first device call."""
    from yat_amd.lib import YatLibraryError
    from yat_amd.optim import FlatAdamW
    model = _stand_in(shard=SimpleNamespace(ddp=None, rank=0, world=2))
    opt = FlatAdamW(model, lr=1e-5, stochastic_rounding=True, use_ema=True)
    with pytest.raises(YatLibraryError, match="device tensors"):
        opt.step()
    assert opt.step_count == 1                        # past the refusal that master_weights meets before anything else


# ------------------------------------------------------------------------------------------------ config key
BASE = "urls:\n  - a.tar\nbatch_size: 2\nlearning_rate: 1e-5\nsteps: 4\nnum_steps_per_validation: 2\nvalidation_prompts:\n  - x\n"


def _read(tmp_path, extra):
    f = tmp_path / "c.yaml"
    f.write_text(BASE + extra)
    return TrainingParameters().read_yaml(str(f))


@pytest.mark.parametrize("text, want", [("true", True), ("1", True), ("yes", True), ("false", False), ("False", False), ("0", False),
                                        ("no", False), ("off", False)])
def test_config_key_is_parsed_like_master_weights(tmp_path, text, want):
    assert _read(tmp_path, f"stochastic_rounding: {text}\n").stochastic_rounding is want
    assert _read(tmp_path, f"master_weights: {text}\n").master_weights is want


def test_config_without_the_key_is_unchanged(tmp_path):
    p = _read(tmp_path, "")
    assert not hasattr(p, "stochastic_rounding")
    with_key = vars(_read(tmp_path, "stochastic_rounding: true\n"))
    assert {k: v for k, v in with_key.items() if k != "stochastic_rounding"} == vars(p)
    for path in sorted(glob.glob(os.path.join(GOLDEN, "config_*.yaml"))):       # the reference's configs parse as before
        golden = json.load(open(path.replace("config_", "params_").replace(".yaml", ".json")))
        assert "stochastic_rounding" not in golden
        assert json.loads(json.dumps(vars(TrainingParameters().read_yaml(path)))) == golden, path


@pytest.mark.parametrize("key, env, want", [(None, None, False), (None, "1", True), (None, "0", False), ("true", None, True),
                                            ("true", "0", True), ("false", "1", False), ("0", "1", False)])
def test_key_wins_over_the_environment_in_make_optimizer(tmp_path, clean_env, key, env, want):
    """``Model.make_optimizer`` hands the key and the dataset seed to FlatAdamW; YAT_STOCHASTIC_ROUNDING decides only when the
    key is absent."""
    from yat_amd.common.trainer import Model, optimizer_arithmetic
    if env is not None:
        clean_env.setenv("YAT_STOCHASTIC_ROUNDING", env)
    params = _read(tmp_path, "dataset_seed: 31\n" + ("" if key is None else f"stochastic_rounding: {key}\nuse_ema: true\n"))
    opt = Model.make_optimizer(SimpleNamespace(params=params), _stand_in())
    assert opt.stochastic_rounding is want and opt.master is None and opt.master_weights is False
    assert opt.exp_avg.dtype == BF and opt.sr_seed == 31
    line = optimizer_arithmetic(opt)
    assert line.startswith("stochastic_rounding (" if want else "bf16")
    if want:
        for words in ("bf16", "fp32", "Philox", "not the reference's arithmetic"):
            assert words in line, words


def test_both_keys_in_one_config_are_refused(tmp_path, clean_env):
    from yat_amd.common.trainer import Model
    params = _read(tmp_path, "master_weights: true\nstochastic_rounding: true\n")
    with pytest.raises(ValueError, match="stochastic_rounding"):
        Model.make_optimizer(SimpleNamespace(params=params), _stand_in())
