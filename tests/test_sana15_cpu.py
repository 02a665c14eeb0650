"""SANA-1.5 (``qk_norm="rms_norm_across_heads"``) without a GPU: parameter layout, config I/O, the refusals of
``from_pretrained``, the argument checks of the segmented RMSNorm entry points, and a known answer for the test reference
itself (tests/sana15_ref.py)."""
import json
import math
import os

import pytest
import torch

from tests.sana15_ref import SanaTransformer15Ref, SelfAttn15, hip_config

BF = torch.bfloat16
NORM_KEYS = ("attn1.norm_q.weight", "attn1.norm_k.weight", "attn2.norm_q.weight", "attn2.norm_k.weight")


def _tiny(**kw):
    from oracle.sana_ref import SanaConfig as RC
    return RC.tiny(**kw)


def test_state_dict_keys_are_the_references():
    """With qk_norm set the device model has exactly the reference's key set and shapes (four more (D,) vectors per block),
    in forward-execution order: the norms sit behind the projections they follow, the fused q|k|v and k|v views still span
    consecutive tensors."""
    from yat_amd.sana import SanaTransformer2DModelHIP
    rc = _tiny(num_layers=2, modified_blocks=[1])
    ref = SanaTransformer15Ref(rc)
    m = SanaTransformer2DModelHIP(hip_config(rc), device="cpu")
    sd, rsd = m.state_dict(), ref.state_dict()
    assert set(sd) == set(rsd), set(sd) ^ set(rsd)
    assert all(sd[k].shape == rsd[k].shape for k in sd)
    assert sum(k.endswith(NORM_KEYS) for k in sd) == 4 * rc.num_layers
    names = list(m.P)
    for i in range(rc.num_layers):
        b = f"transformer_blocks.{i}."
        at = names.index
        assert at(b + "attn1.to_v.weight") + 1 == at(b + "attn1.norm_q.weight") == at(b + "attn1.norm_k.weight") - 1
        assert at(b + "attn1.norm_k.weight") + 1 == at(b + "attn1.to_out.0.weight")
        assert at(b + "attn2.to_v.bias") + 1 == at(b + "attn2.norm_q.weight") == at(b + "attn2.norm_k.weight") - 1
        assert at(b + "attn2.norm_k.weight") + 1 == at(b + "attn2.to_out.0.weight")
    D = rc.inner_dim
    w, _ = m._fused("transformer_blocks.1.attn1.to_q.weight", 3 * D, D)
    assert w.data_ptr() == m.P["transformer_blocks.1.attn1.to_q.weight"].data_ptr()
    assert w[2 * D:].data_ptr() == m.P["transformer_blocks.1.attn1.to_v.weight"].data_ptr()
    wkv, _ = m._fused("transformer_blocks.1.attn2.to_k.weight", 2 * D, D)
    assert wkv[D:].data_ptr() == m.P["transformer_blocks.1.attn2.to_v.weight"].data_ptr()
    m.load_state_dict({k: v.to(BF) for k, v in rsd.items()})
    assert m.bucket_bounds[0][0] == 0 and m.bucket_bounds[-1][1] == m.numel_flat
    assert all(a[1] == b[0] for a, b in zip(m.bucket_bounds, m.bucket_bounds[1:]))


def test_without_qk_norm_the_layout_is_unchanged():
    """qk_norm=None: key list, flat offsets, total and buckets are those of a model that has never heard of the setting --
    pinned against offsets computed here from the spec list of a qk_norm model with the norm entries taken out."""
    from oracle.sana_ref import SanaTransformerRef
    from yat_amd.flat import SHARD_ALIGN
    from yat_amd.sana import SanaConfig, SanaTransformer2DModelHIP, _param_specs
    rc = _tiny(num_layers=3)
    plain = SanaTransformer2DModelHIP(SanaConfig(**{k: getattr(rc, k) for k in SanaConfig.__dataclass_fields__}), device="cpu")
    assert plain.cfg.qk_norm is None and plain.config.qk_norm is None
    specs = [(k, s) for k, s in _param_specs(hip_config(rc)) if not k.endswith(NORM_KEYS)]
    assert [k for k, _ in specs] == list(plain.P) == [k for k, _ in _param_specs(plain.cfg)]
    assert set(plain.P) == set(SanaTransformerRef(rc).state_dict())
    offs, off = [], 0
    for k, shape in specs:                      # FlatParamModule._alloc_flat: 16-byte segments, buckets start at SHARD_ALIGN
        if k.startswith("transformer_blocks.") and k.split(".", 2)[2] == "scale_shift_table":
            off = -(-off // SHARD_ALIGN) * SHARD_ALIGN
        offs.append(off)
        off += -(-math.prod(shape) // 8) * 8
    off = -(-off // SHARD_ALIGN) * SHARD_ALIGN
    assert [plain._offset[k] for k, _ in specs] == offs and plain.numel_flat == off
    starts = [0] + [plain._offset[f"transformer_blocks.{i}.scale_shift_table"] for i in range(rc.num_layers)]
    assert plain.bucket_bounds == [(a, b) for a, b in zip(starts, starts[1:] + [off])]
    assert "qk_norm" not in SanaConfig.__dataclass_fields__        # SANA-1.0 descriptions are walked by these names


def test_config_validation_and_equality():
    from yat_amd.sana import SanaConfig
    a, b = hip_config(_tiny()), hip_config(_tiny())
    assert a == b and a != hip_config(_tiny(), qk_norm=None) and "qk_norm='rms_norm_across_heads'" in repr(a)
    assert a.to_dict()["qk_norm"] == "rms_norm_across_heads" and a.to_dict()["num_layers"] == 2
    bad = hip_config(_tiny(), qk_norm="layer_norm")
    with pytest.raises(ValueError, match="qk_norm"):
        bad.validate()
    SanaConfig(qk_norm="rms_norm_across_heads").validate()          # SANA-1.5-1.6B: D = 2240


def test_config_round_trip(tmp_path):
    from yat_amd.sana import SanaTransformer2DModelHIP
    rc = _tiny(num_layers=1)
    m = SanaTransformer2DModelHIP(hip_config(rc), device="cpu").init_synthetic(3)
    w = m.P["transformer_blocks.0.attn2.norm_k.weight"].float()
    assert 0.5 < w.mean() < 1.5 and w.std() > 0.02                  # 1 + 0.1 randn, not the 0.02 randn of a bias
    m.save_pretrained(str(tmp_path / "m"))
    raw = json.load(open(tmp_path / "m" / "config.json"))
    assert raw["qk_norm"] == "rms_norm_across_heads" and raw["guidance_embeds"] is False
    assert raw["guidance_embeds_scale"] == 0.1 and raw["timestep_scale"] == 1.0
    again = SanaTransformer2DModelHIP.from_pretrained(str(tmp_path / "m"), device="cpu")
    assert again.cfg == m.cfg and again.cfg.qk_norm == "rms_norm_across_heads"
    assert list(again.P) == list(m.P) and torch.equal(again.flat_param, m.flat_param)
    # a SANA-1.0 directory: no 1.5 keys written, the config comes back without the setting
    from yat_amd.sana import SanaConfig
    m0 = SanaTransformer2DModelHIP(SanaConfig(**{k: getattr(rc, k) for k in SanaConfig.__dataclass_fields__}), device="cpu")
    m0.save_pretrained(str(tmp_path / "m0"))
    raw0 = json.load(open(tmp_path / "m0" / "config.json"))
    assert not {"qk_norm", "guidance_embeds", "guidance_embeds_scale", "timestep_scale"} & set(raw0)
    assert SanaTransformer2DModelHIP.from_pretrained(str(tmp_path / "m0"), device="cpu").cfg == m0.cfg


@pytest.mark.parametrize("key,value", [("guidance_embeds", True), ("timestep_scale", 0.001), ("qk_norm", "layer_norm")])
def test_from_pretrained_refuses_by_name(tmp_path, key, value):
    from yat_amd.sana import SanaTransformer2DModelHIP
    m = SanaTransformer2DModelHIP(hip_config(_tiny(num_layers=1)), device="cpu")
    m.save_pretrained(str(tmp_path / "m"))
    path = os.path.join(tmp_path, "m", "config.json")
    raw = json.load(open(path))
    raw[key] = value
    json.dump(raw, open(path, "w"))
    with pytest.raises(ValueError, match=key):
        SanaTransformer2DModelHIP.from_pretrained(str(tmp_path / "m"), device="cpu")
    raw.update({"guidance_embeds": False, "timestep_scale": 1.0, "qk_norm": "rms_norm_across_heads",
                "guidance_embeds_scale": 0.37})                      # ... and guidance_embeds_scale is ignored
    json.dump(raw, open(path, "w"))
    assert SanaTransformer2DModelHIP.from_pretrained(str(tmp_path / "m"), device="cpu").cfg == m.cfg


def test_segmented_rmsnorm_rejects_bad_arguments_without_a_gpu(built_lib):
    """yat_rmsnorm_seg_fwd / _bwd validate before any launch (fake non-null pointers are never dereferenced)."""
    from yat_amd import lib as ylib
    lib = ylib.load()
    P, EINVAL = 0x7f0000001000, -1
    good = dict(M=4, D=64, nseg=2, x=P, ldx=192, w0=P, w1=P, y=P, ldy=192, keep=None, rstd=P, dy=P, lddy=192, dx=P, lddx=192,
                dw0=P, dw1=P, ws=P)

    def fwd(**kw):
        a = {**good, **kw}
        return lib.yat_rmsnorm_seg_fwd(a["M"], a["D"], a["nseg"], 1e-5, a["x"], a["ldx"], a["w0"], a["w1"], a["y"], a["ldy"],
                                       a["keep"], a["rstd"], None)

    def bwd(**kw):
        a = {**good, **kw}
        return lib.yat_rmsnorm_seg_bwd(a["M"], a["D"], a["nseg"], a["x"], a["ldx"], a["w0"], a["w1"], a["rstd"], a["dy"],
                                       a["lddy"], a["dx"], a["lddx"], a["dw0"], a["dw1"], 0, a["ws"], None)

    for bad in (dict(D=60, ldx=184, ldy=184, lddy=184, lddx=184), dict(D=4104, ldx=8208, ldy=8208, lddy=8208, lddx=8208),
                dict(nseg=0), dict(nseg=3, ldx=256, ldy=256, lddy=256, lddx=256), dict(M=0), dict(ldx=196), dict(ldx=120),
                dict(x=None), dict(w0=None), dict(w1=None), dict(rstd=None)):
        assert fwd(**bad) == EINVAL and bwd(**bad) == EINVAL, bad
    for bad in (dict(ldy=196), dict(ldy=120), dict(y=None)):
        assert fwd(**bad) == EINVAL, bad
    for bad in (dict(lddy=196), dict(lddy=64), dict(lddx=196), dict(lddx=120), dict(dy=None), dict(dx=None), dict(dw1=None),
                dict(dw0=None), dict(ws=None)):
        assert bwd(**bad) == EINVAL, bad
    # one fp32 partial row per workgroup and segment; a workgroup takes 16 rows at a time, at most 256 workgroups
    assert lib.yat_rmsnorm_seg_bwd_workspace_bytes(17, 2240, 2) == 2 * 2 * 2240 * 4
    assert lib.yat_rmsnorm_seg_bwd_workspace_bytes(16, 72, 1) == 72 * 4
    assert lib.yat_rmsnorm_seg_bwd_workspace_bytes(8192, 2240, 2) == 2 * 256 * 2240 * 4


def test_reference_attn1_known_answer():
    """The test reference against a hand-written fp64 evaluation of norm -> ReLU -> linear attention (tiny dims, bf16 weights
    and input taken as exact): in fp32 the module agrees to fp32 rounding, and in bf16 -- where q and k carry the two bf16
    roundings of the norm -- a restatement with exactly those roundings agrees to the bf16 rounding of the output alone."""
    torch.manual_seed(0)
    H, C, B, N = 2, 32, 2, 6
    D = H * C
    attn = SelfAttn15(D, H, C)
    with torch.no_grad():
        for p in attn.parameters():
            p.copy_((torch.randn(p.shape) / (math.sqrt(p.shape[-1]) if p.ndim > 1 else 4)).to(BF).float())
        # weights with sign changes: a constant factor on q or k cancels in linear attention, a per-channel one that flips
        # what the ReLU keeps does not
        attn.norm_q.weight.copy_((0.5 + torch.randn(D)).to(BF).float())
        attn.norm_k.weight.copy_((0.5 + torch.randn(D)).to(BF).float())
    x = torch.randn(B, N, D).to(BF)

    def by_hand(rounded):
        rb = (lambda t: t.to(BF).double()) if rounded else (lambda t: t)
        x64 = x.double()
        W = {n: getattr(attn, n).weight.detach().double() for n in ("to_q", "to_k", "to_v")}
        q, k, v = (rb(x64 @ W[n].T) for n in ("to_q", "to_k", "to_v"))

        def norm(t, w):
            r = torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-5)
            return rb(rb(t * r) * w.detach().double())
        q, k = norm(q, attn.norm_q.weight).relu(), norm(k, attn.norm_k.weight).relu()
        out = torch.empty(B, N, D, dtype=torch.float64)
        for b in range(B):
            for h in range(H):
                s = slice(h * C, (h + 1) * C)
                kv = k[b, :, s].T @ v[b, :, s]                    # [C, C]: sum_n k_n v_n^T
                ks = k[b, :, s].sum(0)                            # [C]
                out[b, :, s] = (q[b, :, s] @ kv) / ((q[b, :, s] @ ks)[:, None] + 1e-15)
        out = rb(out)
        return rb(out @ attn.to_out[0].weight.detach().double().T + attn.to_out[0].bias.detach().double())

    got32 = attn.linear_attention(x.float()).double()
    want = by_hand(False)
    assert (got32 - want).abs().max() <= 1e-4 * want.abs().max()
    got_bf = attn.to(BF).linear_attention(x).double()
    want_bf = by_hand(True)
    # bf16 rounding of the output only: 1 ulp (2^-8 relative) per element, plus the same for the rounding of the attention
    # output `o` carried through to_out (|dout| <= 2^-9 * sum |o| |W|, bounded here by 2^-8 of the largest output)
    tol = 2.0 ** -8 * want_bf.abs() + 2.0 ** -8 * want_bf.abs().max()
    assert bool(((got_bf - want_bf).abs() <= tol).all()), (got_bf - want_bf).abs().max()
    # the two norm weights are not interchangeable in this answer
    attn.norm_q.weight, attn.norm_k.weight = attn.norm_k.weight, attn.norm_q.weight
    swapped = attn.linear_attention(x).double()
    assert (swapped - want_bf).abs().max() > 4 * tol.max()
