"""AutoencoderKL encoder host logic without a GPU: config parsing and refusals, the strict loader, argument checks of the new
C-ABI entry points, the restatement's Downsample2D and sampler against written-out torch, the PixArt-Sigma / SD3.5 trainers'
extract_latents without a VAE and the host half of the extraction tool (yat_amd/autoencoder_kl_encoder.py,
yat_amd/extract_latents.py, include/yat_hip.h yat_vae_conv3x3_down / yat_vae_kl_sample)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import autoencoder_kl_encoder_ref as encref
from yat_amd import autoencoder_kl as kl
from yat_amd import autoencoder_kl_encoder as ke
from yat_amd import extract_latents as xl
from yat_amd.common.aspect_ratios import ASPECT_RATIO_512_BIN
from yat_amd.common.shards import read_shard, write_shard

BF = torch.bfloat16
TINY = {"latent_channels": 4, "block_out_channels": [32, 64, 64], "layers_per_block": 2, "norm_num_groups": 8,
        "scaling_factor": 0.5, "shift_factor": None, "use_post_quant_conv": True, "mid_block_add_attention": True}


# ---------------------------------------------------------------------------------------------------------------- config
def test_config_parsing_of_both_families():
    c = ke.parse_encoder_config(encref.diffusers_config(encref.SDXL_KL))
    assert c.block_out_channels == (128, 256, 512, 512) and c.layers_per_block == 2 and c.norm_num_groups == 32
    assert c.latent_channels == 4 and c.moment_channels == 8 and c.in_channels == 3 and c.spatial_factor == 8
    assert c.use_quant_conv and c.mid_block_add_attention and c.shift_factor is None
    assert c.scaling_factor == pytest.approx(0.13025)
    c = ke.parse_encoder_config(encref.diffusers_config(encref.SD35_KL))
    assert c.latent_channels == 16 and c.moment_channels == 32 and not c.use_quant_conv
    assert c.shift_factor == pytest.approx(0.0609) and c.scaling_factor == pytest.approx(1.5305)
    # diffusers' defaults for absent keys
    d = ke.parse_encoder_config({"block_out_channels": [64]})
    assert d.latent_channels == 4 and d.layers_per_block == 1 and d.use_quant_conv and d.spatial_factor == 1
    assert d.scaling_factor == pytest.approx(0.18215)
    # use_quant_conv is read on its own, not from the decoder's switch
    raw = dict(encref.diffusers_config(encref.SDXL_KL), use_quant_conv=False, use_post_quant_conv=True)
    assert not ke.parse_encoder_config(raw).use_quant_conv


@pytest.mark.parametrize("key,value,exc,names", [
    ("down_block_types", ["DownEncoderBlock2D"] * 3 + ["AttnDownEncoderBlock2D"], NotImplementedError, "AttnDownEncoderBlock2D"),
    ("down_block_types", ["DownEncoderBlock2D"] * 3, ValueError, "3 entries"),
    ("act_fn", "gelu", NotImplementedError, "gelu"),
    ("norm_num_groups", 48, NotImplementedError, "norm_num_groups"),
    ("block_out_channels", [128, 256, 512, 256], NotImplementedError, "mid-block width 256"),
    ("latent_channels", 6, NotImplementedError, "latent_channels 6"),
    ("in_channels", 9, NotImplementedError, "9 input channels"),
    ("layers_per_block", 0, NotImplementedError, "layers_per_block"),
])
def test_config_refuses_unbuilt_forms_by_name(key, value, exc, names):
    raw = dict(encref.diffusers_config(encref.SDXL_KL), **{key: value})
    with pytest.raises(exc, match=names):
        ke.parse_encoder_config(raw)


# ---------------------------------------------------------------------------------------------------------------- loader
@pytest.mark.parametrize("cfg", [encref.SDXL_KL, encref.SD35_KL, TINY], ids=["sdxl", "sd35", "tiny"])
def test_expected_keys_are_the_restatements_state_dict(cfg):
    want = ke.expected_keys(ke.parse_encoder_config(encref.diffusers_config(cfg)))
    sd = encref.random_encoder_state(cfg, seed=1)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert ("quant_conv.weight" in want) == cfg["use_post_quant_conv"]
    n = len(cfg["block_out_channels"])
    assert f"encoder.down_blocks.{n - 2}.downsamplers.0.conv.weight" in want
    assert f"encoder.down_blocks.{n - 1}.downsamplers.0.conv.weight" not in want         # none after the last block
    assert ("encoder.down_blocks.1.resnets.0.conv_shortcut.weight" in want) == (cfg["block_out_channels"][0] != cfg["block_out_channels"][1])
    assert "encoder.down_blocks.1.resnets.1.conv_shortcut.weight" not in want            # only a block's first resnet


def test_strict_loader_names_missing_misshaped_extra_and_doubled_keys():
    cfg = ke.parse_encoder_config(encref.diffusers_config(TINY))
    sd = encref.random_encoder_state(TINY, seed=1)
    sd["decoder.conv_in.weight"] = torch.zeros(4)                      # decoder keys are ignored
    sd["post_quant_conv.weight"] = torch.zeros(4)
    packed = ke.pack_weights(cfg, sd)
    assert packed["conv_in.w"].shape == (32, 3, 3, 8) and packed["conv_in.w"].dtype == BF
    assert not packed["conv_in.w"][..., 3:].any()
    assert packed["down_blocks.0.downsamplers.0.conv.w"].shape == (32, 3, 3, 32)
    assert packed["down_blocks.1.resnets.0.sc.w"].shape == (64, 32)
    assert packed["conv_out.w"].shape == (8, 3, 3, 64) and packed["qc.w"].shape == (8, 8)
    assert packed["attn.qkv.w"].shape == (192, 64)
    missing = dict(sd)
    del missing["encoder.mid_block.attentions.0.to_k.weight"]
    with pytest.raises(KeyError, match=r"encoder\.mid_block\.attentions\.0\.to_k\.weight"):
        ke.pack_weights(cfg, missing)
    extra = dict(sd, **{"encoder.down_blocks.2.downsamplers.0.conv.weight": torch.zeros(64, 64, 3, 3)})
    with pytest.raises(KeyError, match=r"encoder\.down_blocks\.2\.downsamplers\.0\.conv\.weight"):
        ke.pack_weights(cfg, extra)
    bad = dict(sd, **{"quant_conv.bias": torch.zeros(4)})
    with pytest.raises(ValueError, match=r"quant_conv\.bias"):
        ke.pack_weights(cfg, bad)
    both = dict(sd, **{"encoder.mid_block.attentions.0.query.weight": sd["encoder.mid_block.attentions.0.to_q.weight"]})
    with pytest.raises(KeyError, match="both its current and its deprecated name"):
        ke.pack_weights(cfg, both)


def test_deprecated_attention_names_pack_the_same():
    cfg = ke.parse_encoder_config(encref.diffusers_config(TINY))
    sd = encref.random_encoder_state(TINY, seed=2)
    old = {}
    for k, v in sd.items():
        for new, dep in (("to_q", "query"), ("to_k", "key"), ("to_v", "value"), ("to_out.0", "proj_attn")):
            tag = f"encoder.mid_block.attentions.0.{new}."
            if k.startswith(tag):
                k = k.replace(tag, f"encoder.mid_block.attentions.0.{dep}.")
                if k.endswith("weight"):
                    v = v.reshape(*v.shape, 1, 1)
        old[k] = v
    assert set(old) != set(sd)
    a, b = ke.pack_weights(cfg, sd), ke.pack_weights(cfg, old)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_encoder_shares_the_decoders_blocks():
    assert issubclass(ke.AutoencoderKLEncoderHIP, kl.KLBlocksHIP) and issubclass(kl.AutoencoderKLDecoderHIP, kl.KLBlocksHIP)
    for name in ("_resnet", "_attention", "_gn"):
        assert name not in vars(ke.AutoencoderKLEncoderHIP) and name not in vars(kl.AutoencoderKLDecoderHIP)
    assert ke.pack_resnet is kl.pack_resnet and ke.resnet_keys is kl.resnet_keys and ke.convert_deprecated is kl.convert_deprecated


# ---------------------------------------------------------------------------------------------------------- entry points
def test_encoder_entry_points_reject_bad_arguments(built_lib):
    from yat_amd import lib as ylib
    lib = ylib.load()
    down = lib.yat_vae_conv3x3_down
    # (B, H, W, Cin, Cout, x, w, bias, y, stream)
    ok = (1, 8, 8, 32, 64, 16, 16, None, 16, None)
    assert down(*((0,) + ok[1:])) == -1                                        # B = 0
    assert down(*(ok[:1] + (7,) + ok[2:])) == -1                               # odd H
    assert down(*(ok[:2] + (9,) + ok[3:])) == -1                               # odd W
    assert down(*(ok[:3] + (12,) + ok[4:])) == -1                              # Cin % 8 != 0
    assert down(*(ok[:4] + (66,) + ok[5:])) == -1                              # Cout % 4 != 0
    assert down(*(ok[:5] + (None,) + ok[6:])) == -1                            # x NULL
    assert down(*(ok[:6] + (None,) + ok[7:])) == -1                            # w NULL
    assert down(*(ok[:8] + (None,) + ok[9:])) == -1                            # y NULL
    assert down(1, 16384, 16384, 8, 8, 16, 16, None, 16, None) == -1           # input > 2 GiB
    samp = lib.yat_vae_kl_sample
    # (B, HW, L, ld, moments, noise, apply_shift, shift, scale, out, stream)
    ok = (1, 64, 4, 8, 16, 16, 0, 0.0, 1.0, 16, None)
    assert samp(*((0,) + ok[1:])) == -1                                        # B = 0
    assert samp(*(ok[:1] + (0,) + ok[2:])) == -1                               # HW = 0
    assert samp(*(ok[:2] + (6, 16) + ok[4:])) == -1                            # L % 4 != 0
    assert samp(*(ok[:2] + (8, 8) + ok[4:])) == -1                             # ld < 2 L
    assert samp(*(ok[:3] + (12,) + ok[4:])) == -1                              # ld % 8 != 0
    assert samp(*(ok[:4] + (None,) + ok[5:])) == -1                            # moments NULL
    assert samp(*(ok[:4] + (24,) + ok[5:])) == -1                              # moments not 16-byte aligned
    assert samp(*(ok[:6] + (2,) + ok[7:])) == -1                               # apply_shift not 0 / 1
    assert samp(*(ok[:9] + (None,) + ok[10:])) == -1                           # out NULL


# ------------------------------------------------------------------------------------------------------ the restatement
def _ramped(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    return x + 0.5 * torch.arange(H).reshape(1, 1, H, 1) - 0.8 * torch.arange(W).reshape(1, 1, 1, W)


def test_restated_downsample_is_pad_right_bottom_then_stride_2():
    x = _ramped(2, 8, 10, 6, 0)
    g = torch.Generator().manual_seed(1)
    w, b = torch.randn(12, 8, 3, 3, generator=g) / 72 ** 0.5, torch.randn(12, generator=g)
    got = encref.downsample(x, w, b)
    assert got.shape == (2, 12, 5, 3)
    assert torch.equal(got, F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2, padding=0))
    # tap (ty, tx) of output pixel (oy, ox) is input pixel (2 oy + ty, 2 ox + tx), zero past the last row / column
    xp = torch.zeros(2, 8, 11, 7)
    xp[:, :, :10, :6] = x
    manual = b.reshape(1, 12, 1, 1) + sum(torch.einsum("bchw,oc->bohw", xp[:, :, ty:ty + 10:2, tx:tx + 6:2], w[:, :, ty, tx])
                                          for ty in range(3) for tx in range(3))
    assert torch.allclose(got, manual, rtol=0, atol=1e-4)
    # the symmetric padding=1 conv (the DC-AE down block's) is a different function: O(1) apart on ramped data
    assert (got - F.conv2d(x, w, b, stride=2, padding=1)).abs().max() > 1.0


@pytest.mark.parametrize("shift", [None, 0.0609])
@pytest.mark.parametrize("with_noise", [True, False])
def test_restated_sampler_is_the_written_out_bf16_arithmetic(shift, with_noise):
    g = torch.Generator().manual_seed(3)
    L, scale = 4, 0.13025
    mom = torch.randn(2, 2 * L, 5, 7, generator=g) * 3
    mom[0, L:, 0, :4] = torch.tensor([-40.0, -30.0, 20.0, 25.0])              # the clamp's edges and beyond
    mom = mom.to(BF)
    noise = torch.randn(2, L, 5, 7, generator=g).to(BF) if with_noise else None
    got = encref.sample(mom, noise, scale, shift)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    mean, logvar = mom[:, :L], mom[:, L:]
    x = mean
    if with_noise:
        lv = logvar.float().clamp(-30.0, 20.0).to(BF)
        std = torch.exp((0.5 * lv.float()).to(BF).float()).to(BF)
        x = (mean.float() + (std.float() * noise.float()).to(BF).float()).to(BF)
    if shift is not None:
        x = (x.float() - f32(shift)).to(BF)
    want = (x.float() * f32(scale)).to(BF)
    assert got.dtype == BF and torch.equal(got, want)
    if with_noise:
        assert got[0, :, 0, :4].isfinite().all()
    # in fp32 the same expression is plain fp32 arithmetic
    m32 = mom.float()
    w32 = m32[:, :L] + (torch.exp(0.5 * m32[:, L:].clamp(-30, 20)) * noise.float() if with_noise else 0)
    w32 = (w32 - f32(shift) if shift is not None else w32) * f32(scale)
    assert torch.equal(encref.sample(m32, noise, scale, shift), w32)


def test_restated_encoder_shapes_and_logvar_range():
    sd = encref.random_encoder_state(TINY, seed=4)
    img = torch.rand(1, 3, 32, 48, generator=torch.Generator().manual_seed(0)) * 2 - 1
    mom = encref.moments(TINY, sd, img, torch.float32)
    assert mom.shape == (1, 8, 8, 12) and mom[:, 4:].abs().max() < 8
    lat = encref.encode(TINY, sd, img, BF, noise=torch.zeros(1, 4, 8, 12))
    assert lat.shape == (1, 4, 8, 12) and lat.dtype == BF


# -------------------------------------------------------------------------------------------------------------- trainers
@pytest.mark.parametrize("module,cls", [("train_pixart_sigma", "PixartSigmaTrainer"), ("train_sd35", "SD35Trainer")])
def test_extract_latents_without_a_vae_names_the_directory(module, cls, tmp_path):
    import importlib
    trainer_cls = getattr(importlib.import_module(module), cls)
    m = trainer_cls.__new__(trainer_cls)                        # host check only: no model, no device
    m.params = SimpleNamespace(pretrained_pipe_path=str(tmp_path / "pipe"))
    m.vae_dir, m.vae_encoder = None, None
    with pytest.raises(NotImplementedError) as e:
        m.extract_latents(torch.zeros(1, 3, 32, 32))
    assert os.path.join(str(tmp_path / "pipe"), "vae") in str(e.value)
    with pytest.raises(NotImplementedError):
        m.extract_embeddings(["a"])


# --------------------------------------------------------------------------------------------------------- extraction tool
def test_encoder_class_follows_the_config(tmp_path, monkeypatch):
    from yat_amd import dcae_encoder
    from tests import dcae_encoder_ref
    made = []
    monkeypatch.setattr(ke.AutoencoderKLEncoderHIP, "from_pretrained", classmethod(lambda c, d, device="cuda": made.append(("KL", d, device)) or "kl"))
    monkeypatch.setattr(dcae_encoder.AutoencoderDCEncoderHIP, "from_pretrained",
                        classmethod(lambda c, d, device="cuda": made.append(("DC", d, device)) or "dc"))
    for name, raw in (("kl", encref.diffusers_config(encref.SD35_KL)),
                      ("dc", dcae_encoder_ref.diffusers_config(dcae_encoder_ref.SANA_F32C32_ENC))):
        d = tmp_path / name
        d.mkdir()
        (d / "config.json").write_text(json.dumps(raw))
        assert kl.load_vae_encoder(str(d), device="cpu") == name
    assert made == [("KL", str(tmp_path / "kl"), "cpu"), ("DC", str(tmp_path / "dc"), "cpu")]


def test_encode_options_per_vae_class():
    assert xl.encode_options("AutoencoderDC", 5, True, True, "cpu") == {}
    o = xl.encode_options("AutoencoderKL", 5, False, False, "cpu")
    assert set(o) == {"generator"} and o["generator"].initial_seed() == 5
    assert xl.encode_options("AutoencoderKL", 5, True, False, "cpu") == {"sample": False}
    o = xl.encode_options("AutoencoderKL", 6, False, True, "cpu")
    assert o["apply_shift"] is False and o["generator"].initial_seed() == 6


class _StubKLEncoder:
    """Stands in for AutoencoderKLEncoderHIP: records its options, returns a latent of the f8 shape."""
    def __init__(self):
        self.seen = []

    def encode_uint8(self, u8, **options):
        self.seen.append((tuple(u8.shape), dict(options)))
        return torch.zeros(1, 16, u8.shape[0] // 8, u8.shape[1] // 8, dtype=BF)


def test_extraction_carries_the_pooled_sidecar_and_the_options(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    paths = []
    for i, (h, w) in enumerate([(90, 150), (128, 128)]):
        p = tmp_path / f"img{i}.png"
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        torch.save(torch.randn(5, 16).to(BF), tmp_path / f"img{i}.emb.pt")
        paths.append(str(p))
    pooled = torch.randn(24).to(BF)
    torch.save(pooled, tmp_path / "img1.pooled.pt")                            # only the second image has one
    stub = _StubKLEncoder()
    samples = list(xl.extract_samples(stub, paths, ASPECT_RATIO_512_BIN, sample=False, apply_shift=False))
    assert stub.seen == [((384, 640, 3), {"sample": False, "apply_shift": False}),
                         ((512, 512, 3), {"sample": False, "apply_shift": False})]
    assert "pooled" not in samples[0] and torch.equal(samples[1]["pooled"], pooled)
    out = tmp_path / "shard-000000.tar"
    write_shard(str(out), samples)
    back = list(read_shard(str(out)))
    assert "pooled.pt" not in back[0] and torch.equal(back[1]["pooled.pt"], pooled)
    assert back[0]["latent.pt"].shape == (16, 48, 80) and back[1]["latent.pt"].shape == (16, 64, 64)
    torch.save(torch.randn(2, 24), tmp_path / "img0.pooled.pt")                # not a [P] vector
    with pytest.raises(ValueError, match=r"img0\.pooled\.pt"):
        list(xl.extract_samples(stub, paths, ASPECT_RATIO_512_BIN))
