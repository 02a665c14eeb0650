"""Plain LoRA above rank 16 without a GPU: the padded-rank rule (R = 8, 16, 32, 64, 128; r > 128 raises), the flat layout
A [R, in] | B^T [R, out] and the peft-layout checkpoint on the CPU stand-in model of tests/test_adapters_layout_cpu.py, and the
argument checks of the three rank-R entry points, which return before any launch.  Every expected number is written out from
the layout rule, none is read back from the class."""
import json
from types import SimpleNamespace

import pytest
import torch

BF16 = torch.bfloat16
TARGETS = ["to_q", "to_k", "to_v", "to_out.0"]
MODULES = ["blocks.0.attn.to_q", "blocks.0.attn.to_k", "blocks.0.attn.to_v", "blocks.0.attn.to_out.0"]
OUT_IN = [(16, 16), (16, 16), (16, 16), (8, 16)]


def _model():
    g = torch.Generator().manual_seed(11)
    flat = torch.randn(1152 + 128 + 16 + 16, generator=g).to(BF16)
    m = SimpleNamespace(flat_param=flat, flat_grad=torch.zeros_like(flat))
    m.P = {"blocks.0.attn.to_q.weight": flat[0:256].view(16, 16),
           "blocks.0.attn.to_k.weight": flat[256:512].view(16, 16),
           "blocks.0.attn.to_v.weight": flat[512:768].view(16, 16),
           "blocks.0.ff.proj.weight": flat[768:1152].view(24, 16),
           "blocks.0.attn.to_out.0.weight": flat[1152:1280].view(8, 16),
           "blocks.0.attn.to_q.bias": flat[1280:1296],
           "blocks.0.attn.norm_q.weight": flat[1296:1312]}
    return m


@pytest.mark.parametrize("r,R", [(20, 32), (48, 64), (128, 128)])
def test_padded_rank_layout_and_checkpoint(r, R, tmp_path):
    from safetensors.torch import load_file
    from yat_amd.lora import LoRAAdapters
    ad = LoRAAdapters(_model(), TARGETS, r=r, alpha=2.0 * r)
    assert (ad.r, ad.R, ad.scale) == (r, R, 2.0)
    off, want = 0, []
    for out, inn in OUT_IN:                                  # A [R, in] | B^T [R, out], target after target
        want.append(dict(oa=off, ob=off + R * inn))
        off += R * (inn + out)
    assert [dict(oa=e["oa"], ob=e["ob"]) for e in ad.entries] == want
    assert [e["module"] for e in ad.entries] == MODULES
    assert ad.numel_flat == off == R * (3 * 32 + 24) and ad.flat_param.shape == (off,) and ad.flat_grad.shape == (off,)
    assert ad.num_parameters() == r * (3 * 32 + 24)          # the unpadded rank
    assert not any(e["pair_ok"] for e in ad.entries)         # in = 16 < the slot of max(64, R) columns
    for e in ad.entries:                                     # the padding rows of A and B^T are zero from the start
        a, bt = ad._views(e, ad.flat_param)
        assert a.shape == (R, e["inn"]) and bt.shape == (R, e["out"])
        assert a[:r].abs().sum() > 0 and not a[r:].any() and not bt.any()
    sd = ad.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == \
        [(f"base_model.model.{m}.{n}", s) for m, (o, i) in zip(MODULES, OUT_IN)
         for n, s in (("lora_A.weight", (r, i)), ("lora_B.weight", (o, r)))]
    flat0 = ad.flat_param.clone()
    sd = {k: v.clone() for k, v in sd.items()}
    ad.flat_param.zero_()
    ad.load_state_dict(sd)
    assert torch.equal(ad.flat_param, flat0)
    ad.save_pretrained(str(tmp_path))
    conf = json.loads((tmp_path / "adapter_config.json").read_text())
    assert conf["r"] == r and conf["peft_type"] == "LORA" and conf["lora_alpha"] == 2.0 * r
    saved = load_file(str(tmp_path / "adapter_model.safetensors"))
    assert sorted(saved) == sorted(sd) and all(torch.equal(saved[k], sd[k]) for k in sd)


def test_rank_limits():
    from yat_amd.lora import LoRAAdapters
    with pytest.raises(NotImplementedError, match="128"):
        LoRAAdapters(_model(), TARGETS, r=129, alpha=129.0)
    assert LoRAAdapters(_model(), TARGETS, r=2, alpha=4.0).R == 8
    assert [LoRAAdapters(_model(), TARGETS, r=r, alpha=1.0).R for r in (8, 9, 16, 17, 32, 33, 64, 65)] == \
        [8, 16, 16, 32, 32, 64, 64, 128]


@pytest.fixture(scope="module")
def lib():
    from yat_amd import lib as ylib
    return ylib.load()


@pytest.mark.parametrize("R", [24, 48, 256])
def test_entry_points_refuse_other_ranks(lib, R):
    """Validation precedes any launch (fake non-null pointers are never dereferenced)."""
    assert lib.yat_rank_expand(16, 64, R, 1, 1, 1, 64, 1.0, 0, None) == -1
    assert lib.yat_lokr_small_wgrad(16, R, 64, 8, 1, 1, 64, 1, 64, 1.0, 0, 1, None) == -1
    assert lib.yat_lora_scatter_b(1, 64, R, 1.0, 1, 1, 1, None) == -1


@pytest.mark.parametrize("R", [32, 64, 128])
def test_entry_points_check_the_other_arguments_at_the_new_ranks(lib, R):
    assert lib.yat_rank_expand(16, 60, R, 1, 1, 1, 64, 1.0, 0, None) == -1                      # N % 8 != 0
    assert lib.yat_rank_expand(16, 64, R, 1, 1, 1, 56, 1.0, 0, None) == -1                      # ldio < N
    assert lib.yat_rank_expand(16, 64, R, 1, 1, None, 64, 1.0, 0, None) == -1                   # no output
    assert lib.yat_lokr_small_wgrad(16, R, 64, R + 1, 1, 1, 64, 1, 64, 1.0, 0, 1, None) == -1   # r_out > R
    assert lib.yat_lokr_small_wgrad(16, R, 64, 8, 1, 1, 32, 1, 64, 1.0, 0, 1, None) == -1       # ldx < N
    assert lib.yat_lokr_small_wgrad(16, R, 64, 8, 1, 1, 64, 1, 64, 1.0, 0, None, None) == -1    # no workspace


@pytest.mark.parametrize("R", [32, 64, 128])
def test_workspace_query(lib, R):
    """Pure host code: positive, monotone in rows, the documented formula G * R * nblk * 128 * 4 with
    G = min(ceil(rows / 128), max(4, 256 / nblk)) -- and bounded: 32 groups at R = 128, N = 11200 would be 180 MB."""
    for N in (8, 136, 2240, 11200):
        nblk = (N + 127) // 128
        sizes = [lib.yat_lokr_small_wgrad_workspace_bytes(rows, R, N) for rows in (1, 100, 129, 777, 4096, 32768, 1 << 20)]
        assert sizes[0] > 0 and sizes == sorted(sizes)
        want = [min((rows + 127) // 128, max(4, 256 // nblk)) * R * nblk * 128 * 4 for rows in (1, 100, 129, 777, 4096, 32768, 1 << 20)]
        assert sizes == want
        assert sizes[-1] <= 32 << 20


def test_workspace_query_unchanged_below_rank_32(lib):
    assert lib.yat_lokr_small_wgrad_workspace_bytes(32768, 8, 2240) == 32 * 8 * 18 * 128 * 4
    assert lib.yat_lokr_small_wgrad_workspace_bytes(32768, 16, 56) == 128 * 16 * 1 * 128 * 4
    assert lib.yat_lokr_small_wgrad_workspace_bytes(300, 8, 56) == 2 * 8 * 1 * 128 * 4
