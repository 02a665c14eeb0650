"""Host layout of the adapter sets that build without the HIP library (LoRA, DoRA, LoHa) on a tiny CPU stand-in model: one
fused q|k|v view, one target outside it, one non-target, rank 2 (padded to R = 8).  Every expected number is written out
from the layout rules in the module docstrings, none is read back from the classes:
    LoRA  per target  A [R, in] | B^T [R, out]
    DoRA  per target  lora_B [out, R] | lora_A [R, in] | magnitude [out]
    LoHa  per target  w1a [out, R] | w1b [R, in] | w2a [out, R] | w2b [R, in]
(LoKr's constructor asks the library for a workspace size: its layout is pinned by tests/test_lokr_gpu.py.)  Written against
the four stand-alone modules before they were folded onto yat_amd/adapters.py, where it passed unchanged."""
import json
import math
from types import SimpleNamespace

import pytest
import torch

BF16 = torch.bfloat16
D, R_, RP = 16, 2, 8                    # width, rank, padded rank
TARGETS = ["to_q", "to_k", "to_v", "to_out.0"]
MODULES = ["blocks.0.attn.to_q", "blocks.0.attn.to_k", "blocks.0.attn.to_v", "blocks.0.attn.to_out.0"]
OUT_IN = [(16, 16), (16, 16), (16, 16), (8, 16)]
W_OFF = [0, 256, 512, 1152]             # q | k | v [16, 16] each, ff.proj [24, 16] (not a target), to_out.0 [8, 16]


def _model():
    g = torch.Generator().manual_seed(11)
    flat = torch.randn(1152 + 128 + 16 + 16, generator=g).to(BF16)
    m = SimpleNamespace(flat_param=flat, flat_grad=torch.zeros_like(flat))
    m.P = {"blocks.0.attn.to_q.weight": flat[0:256].view(16, 16),
           "blocks.0.attn.to_k.weight": flat[256:512].view(16, 16),
           "blocks.0.attn.to_v.weight": flat[512:768].view(16, 16),
           "blocks.0.ff.proj.weight": flat[768:1152].view(24, 16),
           "blocks.0.attn.to_out.0.weight": flat[1152:1280].view(8, 16),
           "blocks.0.attn.to_q.bias": flat[1280:1296],                # a target's bias and a 1-d weight: never adapted
           "blocks.0.attn.norm_q.weight": flat[1296:1312]}
    return m


def _make(kind, model):
    if kind == "lora":
        from yat_amd.lora import LoRAAdapters
        return LoRAAdapters(model, TARGETS, r=R_, alpha=4.0, dropout=0.25, seed=3)
    if kind == "dora":
        from yat_amd.dora import DoRAAdapters
        return DoRAAdapters(model, TARGETS, r=R_, alpha=4.0)
    from yat_amd.loha import LoHaAdapters
    return LoHaAdapters(model, TARGETS, r=R_, alpha=4.0, module_dropout=0.5)


# per kind: entry offset fields, segment starts, size, trainable parameters, checkpoint tensors (name, shape(out, in)),
# adapter_config.json, whether the optimizer gets per-entry ranges
EXPECT = {
    "lora": dict(
        offsets=[dict(oa=0, ob=128), dict(oa=256, ob=384), dict(oa=512, ob=640), dict(oa=768, ob=896)],
        seg_start=[0, 128, 256, 384, 512, 640, 768, 896, 960], numel=960, nparams=3 * 2 * 32 + 2 * 24,
        tensors=[("lora_A.weight", lambda o, i: (R_, i)), ("lora_B.weight", lambda o, i: (o, R_))],
        config={"peft_type": "LORA", "r": 2, "lora_alpha": 4.0, "lora_dropout": 0.25, "target_modules": TARGETS,
                "use_dora": False, "use_rslora": False, "bias": "none", "init_lora_weights": True},
        update_ranges=False),
    "dora": dict(
        offsets=[dict(o=0, n_off=0), dict(o=272, n_off=16), dict(o=544, n_off=32), dict(o=816, n_off=48)],
        seg_start=[0, 128, 256, 272, 400, 528, 544, 672, 800, 816, 880, 1008, 1016], numel=1016,
        nparams=3 * (2 * 32 + 16) + (2 * 24 + 8),
        tensors=[("lora_A.weight", lambda o, i: (R_, i)), ("lora_B.weight", lambda o, i: (o, R_)),
                 ("lora_magnitude_vector.weight", lambda o, i: (o,))],
        config={"peft_type": "LORA", "r": 2, "lora_alpha": 4.0, "lora_dropout": 0.0, "use_dora": True, "use_rslora": False,
                "target_modules": TARGETS, "init_lora_weights": True, "bias": "none"},
        update_ranges=False),
    "loha": dict(
        offsets=[dict(o=0), dict(o=512), dict(o=1024), dict(o=1536)],
        seg_start=[0, 128, 256, 384, 512, 640, 768, 896, 1024, 1152, 1280, 1408, 1536, 1600, 1728, 1792, 1920], numel=1920,
        nparams=3 * 2 * 2 * 32 + 2 * 2 * 24,
        tensors=[("hada_w1_a", lambda o, i: (o, R_)), ("hada_w1_b", lambda o, i: (R_, i)),
                 ("hada_w2_a", lambda o, i: (o, R_)), ("hada_w2_b", lambda o, i: (R_, i))],
        config={"peft_type": "LOHA", "r": 2, "alpha": 4.0, "module_dropout": 0.5, "target_modules": TARGETS,
                "init_weights": True, "rank_dropout": 0.0, "use_effective_conv2d": False},
        update_ranges=True),
}
KINDS = sorted(EXPECT)


def _kaiming(*shape):
    t = torch.empty(shape, dtype=torch.float32)
    torch.nn.init.kaiming_uniform_(t, a=math.sqrt(5))
    return t.to(BF16)


def _init_by_hand(kind, model):
    """The initial flat parameters, drawn tensor by tensor from the global CPU generator in entry order: LoRA A; DoRA A (and
    the magnitude = row norms of W, no draw); LoHa w1_a, w1_b, w2_a.  Padding rows / columns and the other tensors are zero."""
    flat = torch.zeros(EXPECT[kind]["numel"], dtype=BF16)
    for (out, inn), w_off, offs in zip(OUT_IN, W_OFF, EXPECT[kind]["offsets"]):
        if kind == "lora":
            flat[offs["oa"]:offs["oa"] + RP * inn].view(RP, inn)[:R_] = _kaiming(R_, inn)
        elif kind == "dora":
            a0 = offs["o"] + out * RP
            flat[a0:a0 + RP * inn].view(RP, inn)[:R_] = _kaiming(R_, inn)
            w = model.flat_param[w_off:w_off + out * inn].view(out, inn)
            flat[a0 + RP * inn:a0 + RP * inn + out] = torch.linalg.norm(w.float(), dim=1).to(BF16)
        else:
            o = offs["o"]
            flat[o:o + out * RP].view(out, RP)[:, :R_] = _kaiming(out, R_)
            flat[o + out * RP:o + out * RP + RP * inn].view(RP, inn)[:R_] = _kaiming(R_, inn)
            o += out * RP + RP * inn
            flat[o:o + out * RP].view(out, RP)[:, :R_] = _kaiming(out, R_)
    return flat


@pytest.fixture(scope="module", params=KINDS)
def built(request):
    model = _model()
    torch.manual_seed(5)
    ad = _make(request.param, model)
    return request.param, model, ad, ad.flat_param.clone()


def test_entries_and_flat_layout(built):
    kind, model, ad, _ = built
    exp = EXPECT[kind]
    assert model.adapters is ad
    assert [e["module"] for e in ad.entries] == MODULES
    assert [e["key"] for e in ad.entries] == [m + ".weight" for m in MODULES]
    assert [(e["out"], e["inn"]) for e in ad.entries] == OUT_IN
    assert [e["w_off"] for e in ad.entries] == W_OFF
    assert [{k: e[k] for k in offs} for e, offs in zip(ad.entries, exp["offsets"])] == exp["offsets"]
    assert (ad.r, ad.R, ad.scale) == (R_, RP, 2.0)
    assert ad.seg_start.dtype == torch.int64 and ad.seg_start.tolist() == exp["seg_start"]
    assert ad.numel_flat == exp["numel"] and ad.bucket_bounds == [(0, exp["numel"])]
    for t in (ad.flat_param, ad.flat_grad):
        assert t.shape == (exp["numel"],) and t.dtype == BF16
    assert not ad.flat_grad.any()
    assert ad.num_parameters() == exp["nparams"]
    assert ad.param_events is None and ad.grad_ready is None
    assert hasattr(ad, "update_ranges") == exp["update_ranges"]


def test_lookup(built):
    _, model, ad, _ = built
    for base in (model.flat_param, model.flat_grad):
        hit = lambda t: [(e["module"], row) for e, row in ad.lookup(t, base)]
        assert hit(base[0:768].view(48, 16)) == [(MODULES[0], 0), (MODULES[1], 16), (MODULES[2], 32)]       # fused q|k|v
        assert hit(base[256:768].view(32, 16)) == [(MODULES[1], 0), (MODULES[2], 16)]
        assert hit(base[1152:1280].view(8, 16)) == [(MODULES[3], 0)]
        assert hit(base[768:1152].view(24, 16)) == []                                                         # not a target
        assert hit(base[768:1280].view(32, 16)) == [(MODULES[3], 24)]                   # a view that starts before the target
    first = ad.lookup(model.flat_param[0:768].view(48, 16), model.flat_param)
    assert first[0][0] is ad.entries[0]
    assert ad.lookup(model.flat_grad[0:768].view(48, 16), model.flat_grad) is first     # cached per (offset, size)


def test_initial_parameters_follow_the_draw_order(built):
    kind, model, _, flat0 = built
    torch.manual_seed(5)
    assert torch.equal(flat0, _init_by_hand(kind, model))


def test_checkpoint_keys_shapes_and_config(built, tmp_path):
    from safetensors.torch import load_file
    kind, _, ad, flat0 = built
    exp = EXPECT[kind]
    sd = ad.state_dict()
    want = [(f"base_model.model.{m}.{name}", shape(o, i)) for m, (o, i) in zip(MODULES, OUT_IN) for name, shape in exp["tensors"]]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert all(v.dtype == BF16 for v in sd.values())
    sd = {k: v.clone() for k, v in sd.items()}
    ad.flat_param.zero_()
    ad.load_state_dict(sd)
    assert torch.equal(ad.flat_param, flat0)
    ad.save_pretrained(str(tmp_path))
    with open(tmp_path / "adapter_config.json") as f:
        text = f.read()
    assert json.loads(text) == exp["config"] and list(json.loads(text)) == list(exp["config"])
    assert text == json.dumps(exp["config"], indent=2)
    saved = load_file(str(tmp_path / "adapter_model.safetensors"))
    assert sorted(saved) == sorted(sd) and all(torch.equal(saved[k], sd[k]) for k in sd)
