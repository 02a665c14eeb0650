"""FourierFT adapters (``lora_algo: fourierft``) without a GPU: the host-built twiddle table, the two-stage restatement of the
HIP path's arithmetic (tests/fourierft_ref.py) against torch.fft.ifft2 in float64, the host logic of yat_amd/fourierft.py on the
CPU stand-in model of tests/test_adapters_layout_cpu.py, and the argument checks of the two entry points."""
import ctypes as C
import json
import math
from types import SimpleNamespace

import pytest
import torch

from tests import fourierft_ref as R

BF = torch.bfloat16
DIMS = [8, 12, 1152, 2240, 5600, 11200]
EINVAL = -1                                                  # YAT_EINVAL of include/yat_hip.h
EXACT_SHAPES = [(8, 8), (8, 16), (16, 24), (32, 8)]          # (out, in)


def quarter_turn_case(out_dim, in_dim, seed=0):
    """Every position with u in {0, out/4, out/2, 3 out/4} and v likewise, coefficients in -3 .. 3 without zero, in a shuffled
    order: with norm='forward' and scaling 1 every cos / sin the transform meets is 0 or +-1."""
    g = torch.Generator().manual_seed(seed)
    uu = torch.tensor([0, out_dim // 4, out_dim // 2, 3 * out_dim // 4])
    vv = torch.tensor([0, in_dim // 4, in_dim // 2, 3 * in_dim // 4])
    u, v = uu.repeat_interleave(4), vv.repeat(4)
    order = torch.randperm(16, generator=g)
    u, v = u[order], v[order]
    c = torch.randint(1, 4, (16,), generator=g) * (torch.randint(0, 2, (16,), generator=g) * 2 - 1)
    return c.to(BF), u, v


# ---- the table
@pytest.mark.parametrize("d", DIMS)
def test_table_is_correctly_rounded_exact_at_quarter_turns_and_conjugate_symmetric(d):
    from yat_amd.fourierft import twiddle_table
    t = twiddle_table(d)
    assert t.dtype == torch.float32 and t.shape == (d, 2)
    ref = R.table_f64(d)
    # half an fp32 ulp of the float64 value; the float64 value itself carries the rounding of its argument 2 pi m / d (up to
    # 2^-52 * 2 pi absolute) and of libm (an ulp of a double), which is all that matters next to a zero of cos / sin
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23)
    assert ((t.double() - ref).abs() <= 0.5 * ulp + 2.0 ** -49).all()
    if d % 4 == 0:
        assert t[0].tolist() == [1.0, 0.0] and t[d // 4].tolist() == [0.0, 1.0]
        assert t[d // 2].tolist() == [-1.0, 0.0] and t[3 * d // 4].tolist() == [0.0, -1.0]
        assert not torch.signbit(t[[0, d // 4, d // 2, 3 * d // 4]][t[[0, d // 4, d // 2, 3 * d // 4]] == 0]).any()
    m = torch.arange(1, d)
    bits = t.view(torch.int32)
    assert torch.equal(bits[m, 0], bits[d - m, 0])                                         # cos: the same bits
    assert torch.equal(bits[m, 1] & 0x7fffffff, bits[d - m, 1] & 0x7fffffff)               # sin: the same magnitude bits ...
    assert ((t[m, 1] + t[d - m, 1]) == 0).all()                                            # ... and the opposite sign


def test_table_refuses_a_dimension_whose_phases_leave_32_bits():
    from yat_amd.fourierft import twiddle_table
    assert twiddle_table(46340).shape == (46340, 2)
    with pytest.raises(ValueError):
        twiddle_table(46341)


# ---- the two-stage restatement against float64
@pytest.mark.parametrize("out_dim,in_dim", EXACT_SHAPES)
def test_two_stage_restatement_is_exact_on_quarter_turn_inputs(out_dim, in_dim):
    from yat_amd.fourierft import twiddle_table
    c, u, v = quarter_turn_case(out_dim, in_dim)
    truth = R.delta_f64(c, u, v, out_dim, in_dim, "forward", 1.0)
    assert torch.equal(truth, truth.round()) and 0 < truth.abs().max() <= 48
    rows, cols = min(out_dim, in_dim), max(out_dim, in_dim)
    mine = R.two_stage_delta(c, u, v, out_dim, in_dim, "forward", 1.0, twiddle_table(rows), twiddle_table(cols))
    assert mine.dtype == BF and torch.equal(mine.double(), truth)
    # the adjoint on a small-integer d_delta_w: exact integer sums, one bf16 rounding
    dd = torch.randint(-2, 3, (out_dim, in_dim), generator=torch.Generator().manual_seed(1)).to(BF)
    g = R.two_stage_dc(dd, u, v, out_dim, in_dim, "forward", 1.0, twiddle_table(rows), twiddle_table(cols))
    assert torch.equal(g, R.dc_f64(dd, u, v, out_dim, in_dim, "forward", 1.0).to(BF))


@pytest.mark.parametrize("out_dim,in_dim", [(8, 16), (16, 8)])
def test_two_stage_restatement_single_coefficient_within_one_bf16_ulp(out_dim, in_dim):
    """c = 1 at a general (u, v): two nonzero products per output, so the restatement is order-free; its roundings (table,
    s * c, Y, B, the result) must keep it within one bf16 ulp of float64."""
    from yat_amd.fourierft import twiddle_table
    rows, cols = min(out_dim, in_dim), max(out_dim, in_dim)
    tr, tc = twiddle_table(rows), twiddle_table(cols)
    c = torch.ones(1, dtype=BF)
    for uu in range(out_dim):
        for vv in range(in_dim):
            u, v = torch.tensor([uu]), torch.tensor([vv])
            truth = R.delta_f64(c, u, v, out_dim, in_dim, "ortho", 1.0)
            mine = R.two_stage_delta(c, u, v, out_dim, in_dim, "ortho", 1.0, tr, tc).double()
            ulp = torch.exp2(torch.floor(torch.log2(truth.abs().clamp_min(2.0 ** -126))) - 7)
            # next to a zero of the cosine the bound is an ulp of the terms (|s| = 1 / sqrt(out in)), not of their difference
            ulp = torch.maximum(ulp, torch.tensor(2.0 ** (math.floor(math.log2(1.0 / math.sqrt(out_dim * in_dim))) - 7)))
            assert ((mine - truth).abs() <= ulp).all(), (uu, vv)


# ---- host logic
def _model():
    """The stand-in of tests/test_adapters_layout_cpu.py: a fused q|k|v [16, 16] x 3, a non-target, to_out.0 [8, 16]."""
    g = torch.Generator().manual_seed(11)
    flat = torch.randn(1152 + 128 + 16 + 16, generator=g).to(BF)
    m = SimpleNamespace(flat_param=flat, flat_grad=torch.zeros_like(flat))
    m.P = {"blocks.0.attn.to_q.weight": flat[0:256].view(16, 16),
           "blocks.0.attn.to_k.weight": flat[256:512].view(16, 16),
           "blocks.0.attn.to_v.weight": flat[512:768].view(16, 16),
           "blocks.0.ff.proj.weight": flat[768:1152].view(24, 16),
           "blocks.0.attn.to_out.0.weight": flat[1152:1280].view(8, 16),
           "blocks.0.attn.to_q.bias": flat[1280:1296],
           "blocks.0.attn.norm_q.weight": flat[1296:1312]}
    return m


TARGETS = ["to_q", "to_k", "to_v", "to_out.0"]
MODULES = ["blocks.0.attn.to_q", "blocks.0.attn.to_k", "blocks.0.attn.to_v", "blocks.0.attn.to_out.0"]


@pytest.mark.parametrize("out_dim,in_dim,n", [(8, 16, 40), (16, 8, 40), (24, 24, 1), (8, 8, 64)])
def test_csr_is_the_inverse_of_the_position_list(out_dim, in_dim, n):
    from yat_amd.fourierft import build_csr, positions
    u, v = positions(out_dim, in_dim, n)
    row_ptr, col, perm = build_csr(u, v, out_dim, in_dim)
    rows = min(out_dim, in_dim)
    assert all(t.dtype == torch.int32 for t in (row_ptr, col, perm))
    assert row_ptr.shape == (rows + 1,) and row_ptr[0] == 0 and row_ptr[-1] == n and (row_ptr[1:] >= row_ptr[:-1]).all()
    assert sorted(perm.tolist()) == list(range(n))
    back_u, back_v = torch.empty(n, dtype=torch.int64), torch.empty(n, dtype=torch.int64)
    for r in range(rows):
        ents = range(int(row_ptr[r]), int(row_ptr[r + 1]))
        assert [int(perm[e]) for e in ents] == sorted(int(perm[e]) for e in ents)          # a row keeps the coefficients' order
        for e in ents:
            short, long_ = r, int(col[e])
            back_u[perm[e]], back_v[perm[e]] = (short, long_) if out_dim <= in_dim else (long_, short)
    assert torch.equal(back_u, u) and torch.equal(back_v, v)


def test_positions_are_the_seeded_randperm():
    from yat_amd.fourierft import positions
    idx = torch.randperm(16 * 24, generator=torch.Generator().manual_seed(777))[:50]
    u, v = positions(16, 24, 50)
    assert torch.equal(u, idx // 24) and torch.equal(v, idx % 24)
    u2, v2 = positions(16, 24, 50, seed=778)
    assert not (torch.equal(u, u2) and torch.equal(v, v2))
    ru, rv = R.positions(16, 24, 50)
    assert torch.equal(u, ru) and torch.equal(v, rv)


def test_n_follows_from_alpha_and_the_layout_pads_to_eight():
    from yat_amd.fourierft import FourierFTAdapters, n_from_alpha
    assert n_from_alpha(0.01, 2240, 11200) == 250880 and n_from_alpha(0.01, 8, 8) == 1 and n_from_alpha(0.05, 64, 160) == 512
    model = _model()
    ad = FourierFTAdapters(model, TARGETS, alpha=0.05)
    assert model.adapters is ad and [e["module"] for e in ad.entries] == MODULES
    assert [e["n"] for e in ad.entries] == [12, 12, 12, 6]                   # int(0.05 * 256), int(0.05 * 128)
    assert [e["o"] for e in ad.entries] == [0, 16, 32, 48] and ad.numel_flat == 56
    assert ad.seg_start.tolist() == [0, 16, 32, 48, 56] and ad.num_parameters() == 42
    assert not ad.flat_param.any() and not hasattr(ad, "update_ranges")
    assert len(ad._csr) == 2 and sorted(ad._table) == [8, 16] and sorted(ad._B) == [8, 16]
    assert FourierFTAdapters(_model(), TARGETS, n_frequency=9).num_parameters() == 36


def test_exactly_one_of_n_frequency_and_alpha():
    from yat_amd.fourierft import FourierFTAdapters
    with pytest.raises(ValueError, match="exactly one"):
        FourierFTAdapters(_model(), TARGETS)
    with pytest.raises(ValueError, match="exactly one"):
        FourierFTAdapters(_model(), TARGETS, n_frequency=4, alpha=0.1)
    with pytest.raises(ValueError):
        FourierFTAdapters(_model(), TARGETS, n_frequency=129)               # more than to_out.0 has positions
    with pytest.raises(ValueError):
        FourierFTAdapters(_model(), TARGETS, alpha=0.1, norm="unitary")


def test_checkpoint_and_peft_config_round_trip(tmp_path):
    from safetensors.torch import load_file
    from yat_amd.fourierft import FourierFTAdapters
    ad = FourierFTAdapters(_model(), TARGETS, alpha=0.05)
    g = torch.Generator().manual_seed(2)
    for e in ad.entries:
        ad._views(e, ad.flat_param)[0].copy_(torch.randn(e["n"], generator=g).to(BF))
    flat0 = ad.flat_param.clone()
    ad.save_pretrained(str(tmp_path))
    conf = json.load(open(tmp_path / "adapter_config.json"))
    assert conf == {"peft_type": "FOURIERFT", "n_frequency": 1000, "alpha": 0.05,
                    "n_frequency_pattern": dict(zip(MODULES, [12, 12, 12, 6])), "scaling": 1.0, "random_loc_seed": 777,
                    "ifft2_norm": "ortho", "init_weights": True, "target_modules": TARGETS}
    saved = load_file(str(tmp_path / "adapter_model.safetensors"))
    assert sorted(saved) == [f"base_model.model.{m}.fourierft_spectrum" for m in sorted(MODULES)]
    assert [tuple(saved[f"base_model.model.{m}.fourierft_spectrum"].shape) for m in MODULES] == [(12,), (12,), (12,), (6,)]
    again = FourierFTAdapters.from_peft_config(_model(), conf)
    assert again._peft_config() == conf
    again.load_state_dict({k: v.float() for k, v in saved.items()})         # fp32 on load is accepted
    assert torch.equal(again.flat_param, flat0)
    by_n = FourierFTAdapters.from_peft_config(_model(), dict(conf, alpha=None, n_frequency=6))
    assert [e["n"] for e in by_n.entries] == [6, 6, 6, 6]
    with pytest.raises(ValueError, match="coefficients"):
        by_n.load_state_dict(saved)


# ---- ABI
def test_entry_points_reject_bad_arguments_without_a_gpu(built_lib):
    from yat_amd import lib
    L = lib.load()
    p = C.c_void_p(0x1000)                      # never dereferenced: every call below is refused before a launch
    null = C.c_void_p(None)

    def expand(rows=8, cols=16, n=4, row_ptr=p, col=p, perm=p, spec=p, table=p, y=p, ld=16):
        return L.yat_fourier_expand(rows, cols, n, row_ptr, col, perm, spec, 1.0, table, y, ld, None)

    def contract(rows=8, cols=16, n=4, row_ptr=p, col=p, perm=p, z=p, table=p, dc=p, ld=16):
        return L.yat_fourier_contract(rows, cols, n, row_ptr, col, perm, z, ld, 1.0, table, dc, None)

    for fn, ptrs in ((expand, ("row_ptr", "col", "perm", "spec", "table", "y")),
                     (contract, ("row_ptr", "col", "perm", "z", "table", "dc"))):
        for name in ptrs:
            assert fn(**{name: null}) == EINVAL, (fn.__name__, name)
        assert fn(cols=12, ld=16) == EINVAL                         # cols % 8 != 0
        assert fn(cols=0) == EINVAL
        assert fn(n=0) == EINVAL
        assert fn(ld=8) == EINVAL                                   # ld < cols
        assert fn(ld=20) == EINVAL                                  # rows of Y / Z are read and written 16 bytes at a time
        assert fn(rows=0) == EINVAL
        assert fn(cols=46344, ld=46344) == EINVAL                   # (v * k) would leave 32 bits
