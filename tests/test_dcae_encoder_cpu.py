"""DC-AE encoder host logic without a GPU: config parsing, the strict loader, the conv_in channel padding, the down-block
shortcut's index map, argument checks of the new C-ABI entry points, SanaModel.extract_latents without a VAE and the host
half of the extraction tool (yat_amd/dcae_encoder.py, yat_amd/extract_latents.py, include/yat_hip.h yat_dcae_*)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dcae_encoder_ref as enc_ref
from yat_amd import dcae_encoder as de
from yat_amd import extract_latents as xl
from yat_amd.common.aspect_ratios import ASPECT_RATIO_1024_BIN, ASPECT_RATIO_512_BIN
from yat_amd.common.shards import read_shard, write_shard

TINY = {"latent_channels": 8, "block_out_channels": [32, 64, 64], "block_types": ["ResBlock", "EfficientViTBlock",
        "EfficientViTBlock"], "layers_per_block": [2, 1, 1], "scaling_factor": 0.5}


# ---------------------------------------------------------------------------------------------------------------- config
def test_config_scalar_and_list_forms():
    raw = enc_ref.diffusers_config(enc_ref.SANA_F32C32_ENC)
    cfg = de.parse_encoder_config(raw)
    assert cfg.block_out_channels == (128, 256, 512, 512, 1024, 1024)
    assert cfg.block_types == ("ResBlock",) * 3 + ("EfficientViTBlock",) * 3
    assert cfg.layers_per_block == (2, 2, 2, 3, 3, 3)
    assert cfg.qkv_multiscales[3:] == ((5,),) * 3 and cfg.qkv_multiscales[0] == ()
    assert cfg.scaling_factor == pytest.approx(0.41407) and cfg.latent_channels == 32 and cfg.in_channels == 3
    assert cfg.spatial_factor == 32
    scalar = dict(raw, encoder_block_types="EfficientViTBlock", encoder_layers_per_block=2, encoder_qkv_multiscales=[5],
                  encoder_block_out_channels=[64, 64, 128])
    c2 = de.parse_encoder_config(scalar)
    assert c2.block_types == ("EfficientViTBlock",) * 3 and c2.layers_per_block == (2, 2, 2)
    assert c2.qkv_multiscales == ((5,),) * 3 and c2.spatial_factor == 4


@pytest.mark.parametrize("key,value,names", [
    ("downsample_block_type", "pixel_unshuffle", "pixel_unshuffle"),
    ("encoder_layers_per_block", [0, 2, 2, 3, 3, 3], "stage 0"),
    ("encoder_layers_per_block", [2, 2, 0, 3, 3, 3], "stage 2"),
    ("encoder_block_types", "ResBlockX", "ResBlockX"),
    ("encoder_qkv_multiscales", [3], "qkv_multiscales"),
    ("attention_head_dim", 64, "head dim"),
    ("out_shortcut", False, "out_shortcut"),
])
def test_config_refuses_unbuilt_forms_by_name(key, value, names):
    raw = dict(enc_ref.diffusers_config(enc_ref.SANA_F32C32_ENC), **{key: value})
    with pytest.raises(NotImplementedError, match=names):
        de.parse_encoder_config(raw)


def test_config_default_downsample_type_is_the_unbuilt_one():
    raw = enc_ref.diffusers_config(enc_ref.SANA_F32C32_ENC)
    del raw["downsample_block_type"]                          # diffusers' default is "pixel_unshuffle"
    with pytest.raises(NotImplementedError, match="pixel_unshuffle"):
        de.parse_encoder_config(raw)


def test_config_list_length_must_match():
    raw = dict(enc_ref.diffusers_config(enc_ref.SANA_F32C32_ENC), encoder_layers_per_block=[3, 3])
    with pytest.raises(ValueError):
        de.parse_encoder_config(raw)


# ---------------------------------------------------------------------------------------------------------------- loader
def test_strict_loader_names_missing_misshaped_and_extra_keys():
    cfg = de.parse_encoder_config(enc_ref.diffusers_config(TINY))
    sd = enc_ref.random_encoder_state(TINY, seed=1)
    sd["decoder.conv_in.weight"] = torch.zeros(4)             # decoder keys are ignored
    de.check_state(cfg, sd)
    packed = de.pack_weights(cfg, sd)
    assert packed["conv_in.w"].shape == (32, 3, 3, 8) and packed["conv_in.w"].dtype == torch.bfloat16
    assert packed["0.down.w"].shape == (64, 3, 3, 32) and packed["conv_out.w"].shape == (8, 3, 3, 64)
    assert "encoder.down_blocks.0.2.conv.weight" in de.expected_keys(cfg)       # the down block follows the 2 layers
    assert "encoder.down_blocks.2.1.conv.weight" not in de.expected_keys(cfg)   # none after the last stage
    missing = dict(sd)
    del missing["encoder.down_blocks.1.0.attn.to_k.weight"]
    with pytest.raises(KeyError, match=r"encoder\.down_blocks\.1\.0\.attn\.to_k\.weight"):
        de.pack_weights(cfg, missing)
    extra = dict(sd, **{"encoder.down_blocks.0.1.conv3.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match=r"encoder\.down_blocks\.0\.1\.conv3\.weight"):
        de.pack_weights(cfg, extra)
    bad = dict(sd, **{"encoder.down_blocks.0.2.conv.bias": torch.zeros(63)})
    with pytest.raises(ValueError, match=r"encoder\.down_blocks\.0\.2\.conv\.bias"):
        de.pack_weights(cfg, bad)


def test_loader_shares_the_decoders_repack():
    from yat_amd import dcae
    assert de.pack_conv3x3 is dcae.pack_conv3x3 and de.pack_block is dcae.pack_block


def test_conv_in_padding_is_exact():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(16, 3, 3, 3, generator=g)
    b = torch.randn(16, generator=g)
    x = torch.randn(2, 3, 9, 7, generator=g)
    x8 = torch.zeros(2, 8, 9, 7)
    x8[:, :3] = x
    wp = de.pad_conv_in(w)
    assert wp.shape == (16, 8, 3, 3) and torch.equal(wp[:, :3], w) and not wp[:, 3:].any()
    want = F.conv2d(x, w, b, padding=1)
    # the sum in the packed [Cout, 3, 3, 8] order the kernel reads, taken in fp64 so that only the added zeros could differ
    cols = F.unfold(x8.double(), 3, padding=1).reshape(2, 8, 9, 63).permute(0, 3, 2, 1).reshape(2, 63, 72)
    got = (cols @ de.pack_conv3x3(wp).double().reshape(16, 72).T + b.double()).permute(0, 2, 1).reshape(2, 16, 9, 7)
    assert torch.equal(F.conv2d(x8, wp, b, padding=1), want)
    assert torch.allclose(got.float(), want, rtol=0, atol=1e-5)


# --------------------------------------------------------------------------------------------------------- shortcut map
@pytest.mark.parametrize("g", [1, 2, 4, 8])
def test_shortcut_index_map_equals_pixel_unshuffle_mean(g):
    """Gathering by (u // 4, (u % 4) // 2, u % 2) -- the rule yat_dcae_conv3x3_down's epilogue implements -- equals
    pixel_unshuffle(x, 2).unflatten(1, (-1, g)).mean(2) bit for bit, on data without any symmetry."""
    cin = 16
    cout = 4 * cin // g
    gen = torch.Generator().manual_seed(g)
    x = torch.randn(2, cin, 6, 10, generator=gen)
    x += torch.arange(6).reshape(1, 1, 6, 1) * 0.37 + torch.arange(10).reshape(1, 1, 1, 10) * 1.91
    x = x.to(torch.bfloat16).float()     # bf16 values (what the kernel reads): their fp32 sums of <= 8 are exact in any order
    for dt in (torch.float32, torch.bfloat16):
        xd = x.to(dt)
        want = F.pixel_unshuffle(xd, 2).unflatten(1, (-1, g)).mean(dim=2)
        ch, dy, dx = de.shortcut_gather_index(cin, cout)
        assert ch.shape == (cout, g)
        blocks = xd.reshape(2, cin, 3, 2, 5, 2).permute(0, 2, 4, 1, 3, 5)        # [B, oy, ox, C, dy, dx]
        vals = blocks[..., ch, dy, dx]                                           # [B, oy, ox, cout, g]
        got = (vals.float().sum(dim=-1) / g).to(dt).permute(0, 3, 1, 2)          # fp32 accumulation, one rounding
        assert torch.equal(got, want), (g, dt)


# ---------------------------------------------------------------------------------------------------------- entry points
def test_encoder_entry_points_reject_bad_arguments(built_lib):
    from yat_amd import lib as ylib
    lib = ylib.load()
    for fn in (lib.yat_dcae_conv3x3_down, lib.yat_dcae_conv3x3_mean):
        # (B, H, W, Cin, Cout, x, w, bias, shortcut, y, stream)
        ok = (1, 8, 8, 32, 64, 1, 1, None, 0, 1, None)
        assert fn(*((0,) + ok[1:])) == -1                                        # B = 0
        assert fn(*(ok[:3] + (12,) + ok[4:])) == -1                              # Cin % 8 != 0
        assert fn(*(ok[:4] + (66,) + ok[5:])) == -1                              # Cout % 4 != 0
        assert fn(*(ok[:5] + (None,) + ok[6:])) == -1                            # x NULL
        assert fn(*(ok[:6] + (None,) + ok[7:])) == -1                            # w NULL
        assert fn(*(ok[:9] + (None,) + ok[10:])) == -1                           # y NULL
        assert fn(*(ok[:8] + (2,) + ok[9:])) == -1                               # shortcut not 0 / 1
        assert fn(1, 16384, 16384, 8, 8, 1, 1, None, 0, 1, None) == -1           # input > 2 GiB
    down, mean = lib.yat_dcae_conv3x3_down, lib.yat_dcae_conv3x3_mean
    assert down(1, 7, 8, 32, 64, 1, 1, None, 0, 1, None) == -1                   # odd H
    assert down(1, 8, 9, 32, 64, 1, 1, None, 0, 1, None) == -1                   # odd W
    assert down(1, 8, 8, 32, 48, 1, 1, None, 1, 1, None) == -1                   # 4 Cin % Cout != 0
    assert down(1, 8, 8, 8, 64, 1, 1, None, 1, 1, None) == -1                    # Cout > 4 Cin: no whole group
    assert mean(1, 8, 8, 64, 24, 1, 1, None, 1, 1, None) == -1                   # Cin % Cout != 0
    assert mean(1, 8, 8, 32, 64, 1, 1, None, 1, 1, None) == -1                   # Cout > Cin
    assert lib.yat_dcae_image_from_uint8(0, 1, 1, 1, None) == -1
    assert lib.yat_dcae_image_from_uint8(16, None, 1, 1, None) == -1
    assert lib.yat_dcae_image_from_uint8(16, 1, None, 1, None) == -1
    assert lib.yat_dcae_image_from_uint8(16, 1, 1, None, None) == -1


def test_uint8_table_is_totensor_normalize_bf16():
    from yat_amd import ops
    t = ops.dcae_uint8_table("cpu")
    u = torch.arange(256, dtype=torch.uint8)
    want = ((u.float().div(255) - 0.5) / 0.5).to(torch.bfloat16)
    assert t.dtype == torch.bfloat16 and torch.equal(t, want)
    assert t[0] == -1 and t[255] == 1
    # the shortcut form u * (2 / 255) - 1 is not the same function after the bf16 rounding
    assert not torch.equal((u.float() * (2.0 / 255.0) - 1.0).to(torch.bfloat16), want)


# ---------------------------------------------------------------------------------------------------------------- trainer
def test_extract_latents_without_a_vae_names_the_directory(tmp_path):
    import train_sana
    from types import SimpleNamespace
    m = train_sana.SanaModel.__new__(train_sana.SanaModel)      # host check only: no model, no device
    m.params = SimpleNamespace(pretrained_pipe_path=str(tmp_path / "pipe"))
    m.vae_dir, m.vae_encoder = None, None
    with pytest.raises(NotImplementedError) as e:
        m.extract_latents(torch.zeros(1, 3, 32, 32))
    assert os.path.join(str(tmp_path / "pipe"), "vae") in str(e.value)
    with pytest.raises(NotImplementedError):
        m.extract_embeddings(["a"])


# --------------------------------------------------------------------------------------------------------- extraction tool
class _StubEncoder:
    """Stands in for AutoencoderDCEncoderHIP: records what it is given, returns a latent of the f32 shape."""
    def __init__(self):
        self.seen = []

    def encode_uint8(self, u8):
        assert u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[2] == 3
        self.seen.append(tuple(u8.shape))
        h, w = u8.shape[0] // 32, u8.shape[1] // 32
        return torch.full((1, 4, h, w), float(u8.float().mean()) / 255).to(torch.bfloat16)


def _png(path, height, width, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    Image.fromarray(rng.integers(0, 256, (height, width, 3), dtype=np.uint8)).save(path)


def test_bucket_choice_and_resize_size():
    assert xl.bucket_for(ASPECT_RATIO_1024_BIN, 1000, 1000) == ("1.0", 1024, 1024)
    assert xl.bucket_for(ASPECT_RATIO_1024_BIN, 600, 1000) == ("0.6", 768, 1280)
    assert xl.bucket_for(ASPECT_RATIO_1024_BIN, 1750, 1000) == ("1.75", 1344, 768)
    assert xl.bucket_for(ASPECT_RATIO_512_BIN, 300, 1200) == ("0.25", 256, 1024)
    assert xl.bucket_for(ASPECT_RATIO_1024_BIN, 10, 1000)[0] == "0.25"            # beyond the table: the nearest end
    # ties and order: the first key at the smallest distance wins, as the trainer's find_closest_ratio
    assert xl.find_closest_ratio({"0.5": 0, "1.5": 0}, 1.0) == "0.5"


def test_extraction_host_half_round_trips_through_a_shard(tmp_path):
    from PIL import Image
    shapes = [(90, 150), (128, 128), (210, 120)]                                   # h, w: ratios 0.6, 1.0, 1.75
    paths = []
    for i, (h, w) in enumerate(shapes):
        p = tmp_path / f"img{i}.png"
        _png(p, h, w, i)
        torch.save(torch.randn(5 + i, 16).to(torch.bfloat16), tmp_path / f"img{i}.emb.pt")
        paths.append(str(p))
    stub = _StubEncoder()
    samples = list(xl.extract_samples(stub, paths, ASPECT_RATIO_512_BIN, first_key=40))
    assert stub.seen == [(384, 640, 3), (512, 512, 3), (672, 384, 3)]
    assert [s["ratio"] for s in samples] == ["0.6", "1.0", "1.75"]
    assert [s["__key__"] for s in samples] == ["0000040", "0000041", "0000042"]
    # the resize is PIL's bilinear at the bucket size
    key, u8 = xl.resized_uint8(paths[0], ASPECT_RATIO_512_BIN)
    with Image.open(paths[0]) as im:
        want = np.array(im.convert("RGB").resize((640, 384), Image.BILINEAR))
    assert key == "0.6" and np.array_equal(u8.numpy(), want)
    out = tmp_path / "shard-000000.tar"
    write_shard(str(out), samples)
    back = list(read_shard(str(out)))
    assert len(back) == 3
    for s, b, (h, w) in zip(samples, back, [(12, 20), (16, 16), (21, 12)]):
        assert b["ratio"] == float(s["ratio"]) and b["__key__"] == s["__key__"]
        assert b["latent.pt"].shape == (4, h, w) and b["latent.pt"].dtype == torch.bfloat16
        assert torch.equal(b["latent.pt"], s["latent"]) and torch.equal(b["emb.pt"], s["emb"])


def test_missing_sidecar_is_named(tmp_path):
    p = tmp_path / "lonely.png"
    _png(p, 64, 64, 0)
    with pytest.raises(FileNotFoundError, match=r"lonely\.emb\.pt"):
        list(xl.extract_samples(_StubEncoder(), [str(p)], ASPECT_RATIO_512_BIN))
