"""DC-AE decoder host logic without a GPU: config parsing, the strict loader, the q|k|v block permutation against the
restatement's attention processor, the postprocess rounding, argument checks of the new C-ABI entry points and the VAE
lookup of SanaModel (yat_amd/dcae.py, include/yat_hip.h yat_dcae_*)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dcae_ref
from yat_amd import dcae

TINY = {"latent_channels": 8, "block_out_channels": [32, 64, 64], "block_types": ["ResBlock", "EfficientViTBlock",
        "EfficientViTBlock"], "layers_per_block": [1, 1, 1], "scaling_factor": 0.5}


def test_config_scalar_and_list_forms():
    raw = dcae_ref.diffusers_config(dcae_ref.SANA_F32C32)
    cfg = dcae.parse_config(raw)
    assert cfg.block_out_channels == (128, 256, 512, 512, 1024, 1024)
    assert cfg.block_types == ("ResBlock",) * 3 + ("EfficientViTBlock",) * 3
    assert cfg.layers_per_block == (3,) * 6 and cfg.qkv_multiscales[3:] == ((5,),) * 3 and cfg.qkv_multiscales[0] == ()
    assert cfg.scaling_factor == pytest.approx(0.41407) and cfg.latent_channels == 32
    scalar = dict(raw, decoder_block_types="EfficientViTBlock", decoder_layers_per_block=2, decoder_qkv_multiscales=[5],
                  decoder_norm_types="rms_norm", decoder_act_fns="silu", decoder_block_out_channels=[64, 64, 128],
                  latent_channels=32)
    c2 = dcae.parse_config(scalar)
    assert c2.block_types == ("EfficientViTBlock",) * 3 and c2.layers_per_block == (2, 2, 2)
    assert c2.qkv_multiscales == ((5,),) * 3 and c2.norm_types == ("rms_norm",) * 3


@pytest.mark.parametrize("key,value", [("decoder_block_types", "ResBlockX"), ("decoder_norm_types", "batch_norm"),
                                       ("upsample_block_type", "pixel_shuffle"), ("decoder_act_fns", "relu6"),
                                       ("decoder_qkv_multiscales", [3])])
def test_config_refuses_unbuilt_forms(key, value):
    raw = dict(dcae_ref.diffusers_config(dcae_ref.SANA_F32C32), **{key: value})
    with pytest.raises(NotImplementedError):
        dcae.parse_config(raw)


def test_config_list_length_must_match():
    raw = dict(dcae_ref.diffusers_config(dcae_ref.SANA_F32C32), decoder_layers_per_block=[3, 3])
    with pytest.raises(ValueError):
        dcae.parse_config(raw)


def test_strict_loader_names_missing_and_extra_keys():
    cfg = dcae.parse_config(dcae_ref.diffusers_config(TINY))
    sd = dcae_ref.random_state(TINY, seed=1)
    sd["encoder.conv_in.weight"] = torch.zeros(4)             # encoder keys are ignored
    dcae.check_state(cfg, sd)
    packed = dcae.pack_weights(cfg, sd)
    assert packed["conv_in.w"].shape == (64, 3, 3, 8) and packed["conv_in.w"].dtype == torch.bfloat16
    missing = dict(sd)
    del missing["decoder.up_blocks.1.1.attn.to_k.weight"]
    with pytest.raises(KeyError, match=r"decoder\.up_blocks\.1\.1\.attn\.to_k\.weight"):
        dcae.pack_weights(cfg, missing)
    extra = dict(sd, **{"decoder.up_blocks.0.1.conv3.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match=r"decoder\.up_blocks\.0\.1\.conv3\.weight"):
        dcae.pack_weights(cfg, extra)
    bad = dict(sd, **{"decoder.conv_in.bias": torch.zeros(63)})
    with pytest.raises(ValueError, match=r"decoder\.conv_in\.bias"):
        dcae.pack_weights(cfg, bad)


def test_conv_repack_is_tap_major():
    w = torch.randn(5, 16, 3, 3)
    p = dcae.pack_conv3x3(w)
    for co, ky, kx, ci in [(0, 0, 0, 0), (4, 2, 1, 15), (2, 1, 2, 7)]:
        assert p[co, ky, kx, ci] == w[co, ci, ky, kx]


def test_qkv_block_permutation_matches_processor_bitwise():
    """Permuted fused weights -> q | k | v head-major ReLU linear attention written in torch (what yat_linear_attn_fwd
    computes, two calls) -> the restatement's SanaMultiscaleAttnProcessor2_0 output, bit for bit in fp32."""
    C, H, W = 96, 6, 7
    heads = C // 32
    g = torch.Generator().manual_seed(5)
    a = "attn."
    sd = {a + "to_q.weight": torch.randn(C, C, generator=g) / C ** 0.5, a + "to_k.weight": torch.randn(C, C, generator=g) / C ** 0.5,
          a + "to_v.weight": torch.randn(C, C, generator=g) / C ** 0.5,
          a + "to_qkv_multiscale.0.proj_in.weight": torch.randn(3 * C, 1, 5, 5, generator=g) / 5,
          a + "to_qkv_multiscale.0.proj_out.weight": torch.randn(3 * C, 32, 1, 1, generator=g) / 32 ** 0.5}
    x = torch.randn(2, C, H, W, generator=g)
    want = dcae_ref.msla_processor(x, sd, a)

    perm = dcae.qkv_block_perm(heads)
    assert sorted(perm.tolist()) == list(range(3 * heads))
    wcat = torch.cat([sd[a + "to_q.weight"], sd[a + "to_k.weight"], sd[a + "to_v.weight"]], 0)
    wp = dcae.permute_blocks(wcat, perm)
    dw = dcae.permute_blocks(sd[a + "to_qkv_multiscale.0.proj_in.weight"].reshape(3 * C, 25), perm)
    pw = dcae.permute_blocks(sd[a + "to_qkv_multiscale.0.proj_out.weight"].reshape(3 * C, 32), perm)
    qkv = F.linear(x.movedim(1, -1), wp).movedim(-1, 1)                                 # [B, 3C, H, W], q | k | v
    agg = F.conv2d(qkv, dw.reshape(3 * C, 1, 5, 5), padding=2, groups=3 * C)
    agg = F.conv2d(agg, pw.reshape(3 * C, 32, 1, 1), groups=3 * heads)

    def head_major_attention(t):                                                       # t: [B, 3C, H, W]
        B = t.shape[0]
        t = t.reshape(B, 3, heads, 32, H * W)
        q, k, v = F.relu(t[:, 0]), F.relu(t[:, 1]), t[:, 2]
        return dcae_ref.linear_attention(q, k, v).reshape(B, C, H, W)
    got = torch.cat([head_major_attention(qkv), head_major_attention(agg)], 1)
    assert torch.equal(got, want)


def test_postprocess_rounding_on_crafted_values():
    # x -> p = clamp(bf16(bf16(x/2) + 0.5), 0, 1) -> round_half_even(p * 255)
    xs = torch.tensor([-2.0, -1.0, -0.999, 0.0, 1.0, 1.5, 3.0, 2 * (0.5 / 255) - 1, 2 * (1.5 / 255) - 1,
                       2 * (2.5 / 255) - 1, 2 * (127.5 / 255) - 1]).to(torch.bfloat16)
    got = dcae_ref.postprocess(xs.reshape(1, 1, 1, -1)).reshape(-1)
    p = ((xs / 2) + 0.5).clamp(0, 1).float().numpy()
    assert list(got) == list(np.round(p * np.float32(255)).astype(np.uint8))
    assert got[0] == 0 and got[1] == 0 and got[4] == 255 and got[5] == 255 and got[6] == 255 and got[3] == 128


def test_dcae_entry_points_reject_bad_arguments(built_lib):
    from yat_amd import lib as ylib
    lib = ylib.load()
    # yat_dcae_conv3x3(B, H, W, Cin, Cout, up, silu, x, w, bias, sc_mode, sc, sc_ch, res, nchw, y, stream)
    ok = (1, 8, 8, 32, 64, 0, 0, 1, 1, None, 0, None, 0, None, 0, 1, None)
    assert lib.yat_dcae_conv3x3(*((0,) + ok[1:])) == -1                                  # B = 0
    assert lib.yat_dcae_conv3x3(*(ok[:3] + (12,) + ok[4:])) == -1                        # Cin % 8 != 0
    assert lib.yat_dcae_conv3x3(*(ok[:4] + (66,) + ok[5:])) == -1                        # Cout % 4 != 0
    assert lib.yat_dcae_conv3x3(*(ok[:1] + (7,) + ok[2:5] + (1,) + ok[6:])) == -1        # odd H with upsample
    assert lib.yat_dcae_conv3x3(*(ok[:10] + (1, None, 32) + ok[13:])) == -1              # shortcut mode without a source
    assert lib.yat_dcae_conv3x3(*(ok[:10] + (1, 1, 48) + ok[13:])) == -1                 # Cout % shortcut channels
    assert lib.yat_dcae_conv3x3(*(ok[:10] + (3, 1, 32) + ok[13:])) == -1                 # unknown shortcut mode
    assert lib.yat_dcae_conv3x3(*(ok[:14] + (1,) + ok[15:])) == -1                       # NCHW output on the MFMA path
    assert lib.yat_dcae_conv3x3(*(ok[:4] + (3,) + ok[5:10] + (1, 1, 1) + ok[13:])) == -1  # shortcut on the Cout <= 4 path
    assert lib.yat_dcae_conv3x3(*(ok[:7] + (None,) + ok[8:])) == -1                      # x NULL
    assert lib.yat_dcae_msla_aggregate(1, 4, 4, 48, 1, 1, 1, 1, None) == -1              # C3 % 32 != 0
    assert lib.yat_dcae_msla_aggregate(1, 4, 4, 96, None, 1, 1, 1, None) == -1
    assert lib.yat_dcae_rmsnorm_bias(4, 12, 1e-5, 1, 1, 1, None, 0, 1, None) == -1       # D % 8 != 0
    assert lib.yat_dcae_rmsnorm_bias(4, 16, 1e-5, 1, 1, 1, None, 2, 1, None) == -1       # relu not 0 / 1
    assert lib.yat_dcae_rmsnorm_bias(0, 16, 1e-5, 1, 1, 1, None, 0, 1, None) == -1
    assert lib.yat_dcae_image_to_uint8(0, 1, 1, None) == -1
    assert lib.yat_dcae_image_to_uint8(16, None, 1, None) == -1


def test_vae_lookup(tmp_path):
    assert dcae.find_vae_dir(None) is None
    assert dcae.find_vae_dir(str(tmp_path)) is None                                        # no vae/ -> the old path
    (tmp_path / "vae").mkdir()
    assert dcae.find_vae_dir(str(tmp_path)) is None                                        # vae/ without config.json
    (tmp_path / "vae" / "config.json").write_text(json.dumps(dcae_ref.diffusers_config(TINY)))
    assert dcae.find_vae_dir(str(tmp_path)) == os.path.join(str(tmp_path), "vae")


def test_trainer_keeps_the_latent_only_path_without_a_vae(tmp_path):
    """SanaModel wires the decoder only when the pipe directory has vae/config.json (host check, no model built)."""
    import train_sana
    from yat_amd import dit_trainer
    assert issubclass(train_sana.SanaModel, dit_trainer.DiTTrainer) and dit_trainer.find_vae_dir is dcae.find_vae_dir
    assert dcae.find_vae_dir(str(tmp_path / "pipe")) is None
