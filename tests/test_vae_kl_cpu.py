"""AutoencoderKL decoder host logic without a GPU: config parsing, refusal of unbuilt forms, the strict loader, the deprecated
attention names, the latent-channel pad and conv repack, the VAE class dispatch, the SD3.5 pre-scale, argument checks of the
new C-ABI entry points and the PixArt-Sigma / SD3.5 validate() wiring (yat_amd/autoencoder_kl.py, include/yat_hip.h
yat_vae_*)."""
import json
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from tests import autoencoder_kl_ref as klref
from tests import dcae_ref
from yat_amd import autoencoder_kl as kl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = {"latent_channels": 4, "block_out_channels": [32, 64, 64], "layers_per_block": 1, "norm_num_groups": 8,
        "scaling_factor": 0.5, "shift_factor": None, "use_post_quant_conv": True, "mid_block_add_attention": True}


def test_sdxl_and_sd35_configs_parse():
    sdxl = kl.parse_config(klref.diffusers_config(klref.SDXL_KL))
    assert sdxl.latent_channels == 4 and sdxl.latent_padded == 8 and sdxl.use_post_quant_conv
    assert sdxl.block_out_channels == (128, 256, 512, 512) and sdxl.layers_per_block == 2 and sdxl.norm_num_groups == 32
    assert sdxl.scaling_factor == pytest.approx(0.13025) and sdxl.shift_factor is None and sdxl.upsample_factor == 8
    sd35 = kl.parse_config(klref.diffusers_config(klref.SD35_KL))
    assert sd35.latent_channels == 16 and sd35.latent_padded == 16 and not sd35.use_post_quant_conv
    assert sd35.scaling_factor == pytest.approx(1.5305) and sd35.shift_factor == pytest.approx(0.0609)
    assert sd35.mid_block_add_attention
    # diffusers' defaults for absent keys
    bare = kl.parse_config({"block_out_channels": [64, 64], "latent_channels": 4})
    assert bare.use_post_quant_conv and bare.layers_per_block == 1 and bare.norm_num_groups == 32
    assert bare.scaling_factor == pytest.approx(0.18215)


@pytest.mark.parametrize("key,value,name", [
    ("up_block_types", ["UpDecoderBlock2D", "UpDecoderBlock2D", "AttnUpDecoderBlock2D", "UpDecoderBlock2D"],
     "AttnUpDecoderBlock2D"),
    ("act_fn", "gelu", "gelu"),
    ("norm_num_groups", 48, "norm_num_groups"),
    ("block_out_channels", [128, 256, 512, 256], "mid-block width 256"),
    ("out_channels", 4, "out_channels"),
])
def test_config_refuses_unbuilt_forms_by_name(key, value, name):
    raw = dict(klref.diffusers_config(klref.SDXL_KL), **{key: value})
    with pytest.raises(NotImplementedError, match=name):
        kl.parse_config(raw)


def test_mid_width_without_attention_is_built():
    raw = dict(klref.diffusers_config(klref.SDXL_KL), block_out_channels=[128, 256, 256, 256], mid_block_add_attention=False)
    assert kl.parse_config(raw).block_out_channels[-1] == 256


def test_strict_loader_names_missing_and_extra_keys():
    cfg = kl.parse_config(klref.diffusers_config(TINY))
    sd = klref.random_state(TINY, seed=1)
    sd["encoder.conv_in.weight"] = torch.zeros(4)             # encoder / quant_conv keys are ignored
    sd["quant_conv.weight"] = torch.zeros(8, 8, 1, 1)
    assert set(kl.expected_keys(cfg)) == {k for k in sd if k.startswith(("decoder.", "post_quant_conv."))}
    packed = kl.pack_weights(cfg, sd)
    assert packed["conv_in.w"].shape == (64, 3, 3, 8) and packed["conv_in.w"].dtype == torch.bfloat16
    missing = dict(sd)
    del missing["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"]
    with pytest.raises(KeyError, match=r"decoder\.up_blocks\.2\.resnets\.0\.conv_shortcut\.weight"):
        kl.pack_weights(cfg, missing)
    nopqc = {k: v for k, v in sd.items() if not k.startswith("post_quant_conv.")}
    with pytest.raises(KeyError, match=r"post_quant_conv\.weight"):
        kl.pack_weights(cfg, nopqc)
    extra = dict(sd, **{"decoder.up_blocks.0.resnets.2.conv1.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match=r"decoder\.up_blocks\.0\.resnets\.2\.conv1\.weight"):
        kl.pack_weights(cfg, extra)
    cfg_no = kl.parse_config(dict(klref.diffusers_config(TINY), use_post_quant_conv=False))
    with pytest.raises(KeyError, match=r"post_quant_conv\.bias|post_quant_conv\.weight"):
        kl.pack_weights(cfg_no, sd)                            # unconsumed post_quant_conv.* keys
    bad = dict(sd, **{"decoder.conv_in.bias": torch.zeros(63)})
    with pytest.raises(ValueError, match=r"decoder\.conv_in\.bias"):
        kl.pack_weights(cfg, bad)


def test_deprecated_attention_names_pack_bit_exact():
    cfg = kl.parse_config(klref.diffusers_config(TINY))
    sd = klref.random_state(TINY, seed=2)
    old = {}
    for k, v in sd.items():
        for new, dep in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
            tag = f"attentions.0.{new}."
            if tag in k:
                k = k.replace(tag, f"attentions.0.{dep}.")
                if k.endswith("weight") and dep in ("query", "proj_attn"):
                    v = v.reshape(*v.shape, 1, 1)              # one 1x1-conv-shaped tensor form, one Linear form
        old[k] = v
    a, b = kl.pack_weights(cfg, sd), kl.pack_weights(cfg, old)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    both = dict(sd, **{"decoder.mid_block.attentions.0.query.weight": sd["decoder.mid_block.attentions.0.to_q.weight"]})
    with pytest.raises(KeyError, match="to_q"):
        kl.pack_weights(cfg, both)


def test_latent_pad_and_conv_repack_are_exact():
    cfg = kl.parse_config(klref.diffusers_config(TINY))
    sd = klref.random_state(TINY, seed=3)
    p = kl.pack_weights(cfg, sd)
    w = sd["decoder.conv_in.weight"].to(torch.bfloat16)
    assert p["conv_in.w"].shape == (64, 3, 3, 8)
    assert torch.equal(p["conv_in.w"][..., :4], w.permute(0, 2, 3, 1)) and (p["conv_in.w"][..., 4:] == 0).all()
    pq = p["pqc.w"]
    assert pq.shape == (8, 8) and torch.equal(pq[:4, :4], sd["post_quant_conv.weight"].reshape(4, 4).to(torch.bfloat16))
    assert (pq[4:] == 0).all() and (pq[:, 4:] == 0).all() and (p["pqc.b"][4:] == 0).all()
    # the padded computation, in fp32 on bf16 values, is the unpadded one exactly (zeros add exact zeros)
    z = torch.randn(1, 4, 5, 6).to(torch.bfloat16).float()
    zp = kl.pad_latent_channels(z, 8, 1)
    q = F.conv2d(zp, pq.float().reshape(8, 8, 1, 1), p["pqc.b"].float())
    q_ref = F.conv2d(z, sd["post_quant_conv.weight"].to(torch.bfloat16).float(), sd["post_quant_conv.bias"].to(torch.bfloat16).float())
    assert torch.equal(q[:, :4], q_ref) and (q[:, 4:] == 0).all()
    y = F.conv2d(q, p["conv_in.w"].float().permute(0, 3, 1, 2), padding=1)
    y_ref = F.conv2d(q_ref, w.float(), padding=1)
    assert torch.allclose(y, y_ref, rtol=0, atol=1e-6)
    for co, ky, kx, ci in [(0, 0, 0, 0), (63, 2, 1, 3), (7, 1, 2, 2)]:
        assert p["conv_in.w"][co, ky, kx, ci] == w[co, ci, ky, kx]
    qkv = p["attn.qkv.w"]
    a = "decoder.mid_block.attentions.0."
    assert torch.equal(qkv, torch.cat([sd[a + t + ".weight"] for t in ("to_q", "to_k", "to_v")], 0).to(torch.bfloat16))


def test_vae_class_dispatch(tmp_path, monkeypatch):
    assert kl.vae_class(klref.diffusers_config(TINY)) == "AutoencoderKL"
    assert kl.vae_class(dcae_ref.diffusers_config(dcae_ref.SANA_F32C32)) == "AutoencoderDC"
    nokl = {k: v for k, v in klref.diffusers_config(TINY).items() if k != "_class_name"}
    nodc = {k: v for k, v in dcae_ref.diffusers_config(dcae_ref.SANA_F32C32).items() if k != "_class_name"}
    assert kl.vae_class(nokl) == "AutoencoderKL" and kl.vae_class(nodc) == "AutoencoderDC"
    with pytest.raises(NotImplementedError, match="AutoencoderTiny"):
        kl.vae_class({"_class_name": "AutoencoderTiny"})
    from yat_amd import dcae
    seen = []
    monkeypatch.setattr(kl.AutoencoderKLDecoderHIP, "from_pretrained", classmethod(lambda c, d, device: seen.append(("kl", d))))
    monkeypatch.setattr(dcae.AutoencoderDCDecoderHIP, "from_pretrained", classmethod(lambda c, d, device: seen.append(("dc", d))))
    for name, raw in (("kl", nokl), ("dc", dcae_ref.diffusers_config(dcae_ref.SANA_F32C32))):
        d = tmp_path / name
        d.mkdir()
        (d / "config.json").write_text(json.dumps(raw))
        kl.load_vae_decoder(str(d), device="cpu")
    assert seen == [("kl", str(tmp_path / "kl")), ("dc", str(tmp_path / "dc"))]


def test_sd35_pre_scale_applies_no_shift():
    """The SD3.5 reference decodes ``latent / scaling_factor`` (train_sd35.py:155) without adding ``shift_factor`` back."""
    cfg = kl.parse_config(klref.diffusers_config(klref.SD35_KL))
    assert cfg.shift_factor == pytest.approx(0.0609)
    lat = torch.randn(1, 16, 4, 4).to(torch.bfloat16)
    got = kl.pre_scale(lat, cfg)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, (lat.float() / 1.5305).to(torch.bfloat16))
    assert not torch.equal(got, (lat.float() / 1.5305 + 0.0609).to(torch.bfloat16))
    assert torch.equal(got, klref.pre_scale(klref.SD35_KL, lat, torch.bfloat16))


def test_restatement_mid_attention_is_one_head_sdpa():
    """The restatement's Attention (one head of C) against an explicit softmax in fp64."""
    C, H, W = 16, 3, 5
    g = torch.Generator().manual_seed(0)
    a = "attn."
    sd = {a + "group_norm.weight": torch.ones(C), a + "group_norm.bias": torch.zeros(C)}
    for t in ("to_q", "to_k", "to_v", "to_out.0"):
        sd[a + t + ".weight"] = torch.randn(C, C, generator=g) / C ** 0.5
        sd[a + t + ".bias"] = 0.1 * torch.randn(C, generator=g)
    x = torch.randn(1, C, H, W, generator=g)
    got = klref.attention(x.double(), {k: v.double() for k, v in sd.items()}, a, 4)
    h = F.group_norm(x.double(), 4, eps=1e-6).reshape(C, H * W).T
    q, k, v = [h @ sd[a + t + ".weight"].double().T + sd[a + t + ".bias"].double() for t in ("to_q", "to_k", "to_v")]
    o = torch.softmax(q @ k.T / C ** 0.5, -1) @ v
    o = o @ sd[a + "to_out.0.weight"].double().T + sd[a + "to_out.0.bias"].double()
    assert torch.allclose(got, o.T.reshape(1, C, H, W) + x.double(), atol=1e-12)


def test_vae_kl_entry_points_reject_bad_arguments(built_lib):
    from yat_amd import lib as ylib
    lib = ylib.load()
    A = 1 << 12                                                 # a fake, aligned, non-null pointer (never dereferenced)
    # yat_vae_groupnorm(B, HW, C, G, eps, x, w, b, silu, y, workspace, stream)
    ok = (1, 64, 128, 32, 1e-6, A, A, A, 0, A, A, None)
    assert lib.yat_vae_groupnorm(*((0,) + ok[1:])) == -1                                   # B = 0
    assert lib.yat_vae_groupnorm(*(ok[:2] + (120,) + ok[3:])) == -1                        # C % G != 0
    assert lib.yat_vae_groupnorm(*(ok[:2] + (36, 4) + ok[4:])) == -1                       # C % 8 != 0
    assert lib.yat_vae_groupnorm(*(ok[:2] + (4096, 32) + ok[4:])) == -1                    # C > 2048
    assert lib.yat_vae_groupnorm(*(ok[:8] + (2,) + ok[9:])) == -1                          # silu not 0 / 1
    assert lib.yat_vae_groupnorm(*(ok[:10] + (None, None))) == -1                          # null workspace
    assert lib.yat_vae_groupnorm(*(ok[:5] + (None,) + ok[6:])) == -1                       # null x
    assert lib.yat_vae_groupnorm(*(ok[:5] + (A + 2,) + ok[6:])) == -1                      # misaligned x
    assert lib.yat_vae_groupnorm_workspace_bytes(1, 1024 * 1024, 256, 32) == (2048 * 32 * 2 + 32 * 4) * 4
    assert lib.yat_vae_groupnorm_workspace_bytes(2, 100, 64, 32) == (2 * 1 * 32 * 2 + 2 * 32 * 4) * 4
    # yat_vae_attn_fwd(B, N, dh, q, k, v, ld, out, ldo, stream)
    ok = (1, 64, 512, A, A, A, 1536, A, 512, None)
    for dh in (32, 128, 256, 511, 1024):
        assert lib.yat_vae_attn_fwd(*(ok[:2] + (dh,) + ok[3:6] + (3 * dh,) + ok[7:8] + (dh, None))) == -1, dh
    assert lib.yat_vae_attn_fwd(*((1, 0) + ok[2:])) == -1                                 # N = 0
    assert lib.yat_vae_attn_fwd(*(ok[:6] + (500,) + ok[7:])) == -1                        # ld < dh
    assert lib.yat_vae_attn_fwd(*(ok[:6] + (1540,) + ok[7:])) == -1                       # ld % 8 != 0
    assert lib.yat_vae_attn_fwd(*(ok[:3] + (None,) + ok[4:])) == -1                       # null q
    assert lib.yat_vae_attn_fwd(*(ok[:7] + (None,) + ok[8:])) == -1                       # null out
    assert lib.yat_vae_attn_fwd(*(ok[:4] + (A + 8,) + ok[5:])) == -1                      # misaligned k


# ------------------------------------------------------------------------------------------------ trainer validate() wiring
def _fake_trainer(cls, tmp_path, vae_dir, side):
    out = cls.__new__(cls)                                      # host check only: no model, no device
    out.__dict__.update(
        params=types.SimpleNamespace(local_shard_paths=[str(tmp_path / "shard-000000.tar")], validation_prompts=["a red fox"]),
        accelerator=types.SimpleNamespace(device="cpu"), global_step=7, logger=None, vae_dir=vae_dir, vae=None,
        model=types.SimpleNamespace(config=types.SimpleNamespace(sample_size=side), cfg=types.SimpleNamespace(sample_size=side)),
        scheduler=None)
    return out


class _FakeDecoder:
    def __init__(self):
        self.calls = []

    def decode(self, lat):
        self.calls.append(tuple(lat.shape))
        return torch.zeros(lat.shape[0], 3, 8 * lat.shape[2], 8 * lat.shape[3], dtype=torch.bfloat16)

    @staticmethod
    def to_uint8(img):
        return torch.zeros(img.shape, dtype=torch.uint8)


@pytest.mark.parametrize("module,cls,sampler,channels", [("train_pixart_sigma", "PixartSigmaTrainer", "sample_latents_pixart", 4),
                                                         ("train_sd35", "SD35Trainer", "sample_latents_sd3", 16)])
def test_trainers_decode_only_with_a_vae_dir(tmp_path, monkeypatch, module, cls, sampler, channels):
    """validate() without a VAE directory keeps the latent-only path (latents saved, no decoder built, no PNG); with one it
    builds the decoder once (load_vae_decoder) and writes models/<step>/validation_{idx}.png after the latents."""
    sys.path.insert(0, ROOT)
    trainer_cls = getattr(__import__(module), cls)
    from yat_amd import dit_trainer, sampler as smp
    side = 4
    monkeypatch.setattr(smp, sampler, lambda *a, **k: torch.randn(1, channels, side, side).to(torch.bfloat16))
    torch.save([tuple(torch.zeros(1, 2) for _ in range(4))], tmp_path / "validation_embeds.pt")
    monkeypatch.chdir(tmp_path)
    validate = trainer_cls.validate
    built = []
    dec = _FakeDecoder()
    monkeypatch.setattr(dit_trainer, "load_vae_decoder", lambda d, device: built.append(d) or dec)

    t = _fake_trainer(trainer_cls, tmp_path, None, side)
    out = validate(t)
    assert len(out) == 1 and (tmp_path / "models" / "7" / "validation_latents.pt").exists()
    assert not (tmp_path / "models" / "7" / "validation_0.png").exists() and built == [] and t.vae is None

    t = _fake_trainer(trainer_cls, tmp_path, str(tmp_path / "vae"), side)
    validate(t)
    validate(t)
    assert built == [str(tmp_path / "vae")] and t.vae is dec and dec.calls == [(1, channels, side, side)] * 2
    assert (tmp_path / "models" / "7" / "validation_0.png").read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


def test_trainers_look_up_the_vae_like_sana():
    sys.path.insert(0, ROOT)
    import train_pixart_sigma
    import train_sd35
    from yat_amd import dcae, dit_trainer
    for cls in (train_pixart_sigma.PixartSigmaTrainer, train_sd35.SD35Trainer):        # the lookup lives in the shared base
        assert issubclass(cls, dit_trainer.DiTTrainer) and cls.validate is dit_trainer.DiTTrainer.validate
    assert dit_trainer.find_vae_dir is dcae.find_vae_dir and dit_trainer.load_vae_decoder is kl.load_vae_decoder
